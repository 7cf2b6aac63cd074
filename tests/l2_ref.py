"""The contract of mvin_gather_attn_l2_fwd (include/mvin_hip.h, "Two deepest levels in one pass"), plain: torch indexing on the PLAIN
adjacency, in float64 -- or, with ``dtype=torch.float32``, the same formulas op by op in fp32, which is the yardstick of
tests/test_gpu_l2_f64.py.  Nothing here is shared with the code under test: no projected table, no encoded slot word, no per-entity sum.

For every parent i (entity x = parent_ids[i] read as its low 32-bit word, unsigned, clamped to n_entity - 1; query row b = i //
parents_per_pair) with children x1[n] = adj_e[x, n] and grandchildren y[n, k] = adj_e[x1[n], k]:

    p[n, :]  = slot weights of t0 over adj_r[x1[n], :]          softmax of the relations' logits -- or ONES without a logit table (the
                                                                plain mean of aggregators.py:148-152), NOT a softmax of zeros
    S[n]     = sum_k p[n, k] table[y[n, k]]
    with W1, W2:   c1 = q[b] W1 + b1,  c2 = q[b] W2 + b2
                   self1[n] = table[x1[n]] W1 + c1
                   Z[n]     = self1[n] + (S[n] W2 + (sum_k p[n, k]) c2) / K
    W1 = W2 = None (User_orient off: the levels stay raw embeddings; q, b1, b2 are not read):
                   self1[n] = table[x1[n]]
                   Z[n]     = self1[n] + S[n] / K
    out1[n]  = relu(Z[n] A0 + a0)
    p0, p1   = slot weights of t0 / t1 over adj_r[x, :]
    nagg0    = (1 / K) sum_n p0[n] self1[n]          nagg1 = (1 / K) sum_n p1[n] out1[n]
    probs_parent = p0 [P, K],  probs_child = p [P * K, K]       (None without t0: the entry point refuses them then)

A bias that is None counts as zero; t0 and t1 are absent independently.  A bf16 table widens exactly (``.to(dtype)``).  Parents are
evaluated in chunks so that no temporary holds more than 2^26 elements (one parent's grandchildren are K x K x D of them, the
terms of its children's products K x D x D), and no operation mixes parents: every chunking gives the same bits.

``magnitude=True``: every value (table, matrices, biases, queries) enters with its ABSOLUTE value, the slot weights stay what they
are and the ReLU is left out (it is 1-Lipschitz): each output is then the sum of the absolute values of the terms that make it up,
the precondition of the exact cases (magnitude x denominator < 2^24).
"""
import torch

from fold_ref import clamp_ids, slot_weights


def default_chunk(K, D):
    return max(1, (1 << 26) // (K * D * max(K, D)))


def _mm(x, W):
    """x . W as a broadcast product summed over the inner index: a row's bits then do not depend on how many rows are multiplied at once
    (a library GEMM picks its blocking by the row count), so any chunking of the parents gives the same result."""
    return (x.unsqueeze(-1) * W).sum(-2)


def l2_reference(table, adj_e, adj_r, parent_ids, t0, t1, W1, W2, b1, b2, q, A0, a0, B, parents_per_pair, K, dtype=torch.float64,
                 chunk=None, magnitude=False, parts=False):
    """-> nagg0 [P, D], nagg1 [P, D], probs_parent [P, K] | None, probs_child [P * K, K] | None  (P = B * parents_per_pair);
    ``parts``: a fifth value, dict(out1 [P, K, D], self1 [P, K, D], child_rel [P, K, K])."""
    P = B * parents_per_pair
    n_entity, D = table.shape
    assert adj_e.shape[1] == K and parent_ids.shape[0] == P and (W1 is None) == (W2 is None)
    assert W1 is None or q.shape[0] == B
    ab = (lambda t: t.abs()) if magnitude else (lambda t: t)
    f = lambda t: ab(t.to(dtype))                             # noqa: E731
    z = lambda t: 0 if t is None else f(t)                    # noqa: E731
    E = f(table)
    x_all = clamp_ids(parent_ids, n_entity)
    chunk = chunk or default_chunk(K, D)
    n0, n1, pp, pc, keep = [], [], [], [], {"out1": [], "self1": [], "child_rel": []}
    for lo in range(0, P, chunk):
        x = x_all[lo:lo + chunk]
        x1 = adj_e[x].long()                                  # [c, K]    children
        y = adj_e[x1].long()                                  # [c, K, K] grandchildren
        rel = adj_r[x1]
        p = slot_weights(t0, rel, dtype)                      # [c, K, K]
        S = (p[..., None] * E[y]).sum(2)                      # [c, K, D]
        if W1 is not None:
            b = torch.arange(lo, lo + x.shape[0], device=x.device) // parents_per_pair
            qb = f(q[b])
            c1 = _mm(qb, f(W1)) + z(b1)
            c2 = _mm(qb, f(W2)) + z(b2)
            self1 = _mm(E[x1], f(W1)) + c1[:, None, :]
            Z = self1 + (_mm(S, f(W2)) + p.sum(-1, keepdim=True) * c2[:, None, :]) / K
        else:
            self1 = E[x1]
            Z = self1 + S / K
        pre = _mm(Z, f(A0)) + z(a0)
        out1 = pre if magnitude else torch.relu(pre)
        p0 = slot_weights(t0, adj_r[x], dtype)                # [c, K]
        p1 = slot_weights(t1, adj_r[x], dtype)
        n0.append((p0[..., None] * self1).sum(1) / K)
        n1.append((p1[..., None] * out1).sum(1) / K)
        if t0 is not None:
            pp.append(p0)
            pc.append(p.reshape(-1, K))
        if parts:
            keep["out1"].append(out1), keep["self1"].append(self1), keep["child_rel"].append(rel)
    res = (torch.cat(n0), torch.cat(n1), torch.cat(pp) if pp else None, torch.cat(pc) if pc else None)
    return res + ({k: torch.cat(v) for k, v in keep.items()},) if parts else res
