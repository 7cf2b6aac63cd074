"""The contract of mvin_score_small_fwd (include/mvin_hip.h, "The same pass as ONE KERNEL LAUNCH"), plain: the three references the
separate kernels are pinned to, composed -- keyaddr_ref.keyaddr_reference (ripple-set reads and the user MLP, model.py:161-240), then
l2_ref.l2_reference with one parent per pair and q = user_o (the two deepest levels, :259-305), then fold_ref.tail_reference (the mix-hop
tail and the score, :286-317, :158-159) -- in float64, or with ``dtype=torch.float32`` the same chain op by op in fp32: the YARDSTICK of
tests/test_gpu_small_f64.py.  Nothing here is shared with the code under test: plain torch indexing on the PLAIN adjacency.

ONE-HOP TREES (depth = 1; model.py:286-317 with h_hop = 1): the children have no lists and aggregator (1,0) does not exist,
    self1[n] = (E[x1[n]] + q) W1 + b1        (raw E[x1[n]] without W1)
    nagg0    = (1 / K) sum_n p0[n] self1[n]                      p0 = slot weights of t0 over adj_r[x, :] (ones without t0)
    ev0      = (E[x] + q) W0 + b0            (raw E[x] without W0)
    out0     = relu((ev0 + nagg0) A0 + a0)
    item     = [ev0 | out0] Wmix + bmix      Wmix [2D, D]
W2 / b2 / A1 / a1 / t1 are not read.

IDS, as the kernel reads them (clamp_item_ids, clamp_words, clamp_users):
    items          read whole as unsigned 64-bit numbers, clamped to n_entity - 1: a negative id or one with a high word set reads the
                   LAST row
    memory ids     heads and tails are 32-bit words clamped unsigned to n_entity - 1 (negative: the last row)
    relation ids   the ripple sets' and the adjacency's, unsigned words clamped to nR - 1; an adjacency without relations reads 0
    user ids       clamped SIGNED into [0, n_user): negative -> user 0
The adjacency's entity ids are clamped like the memory ids.

``magnitude=True``: every value enters with its absolute value, the attention weights stay what they are and the ReLUs are left out: each
output is then the sum of the absolute values of its terms -- the precondition of the exact cases (magnitude x denominator < 2^24).
"""
import types

import torch

from fold_ref import slot_weights, tail_reference
from keyaddr_ref import keyaddr_reference
from l2_ref import l2_reference


def clamp_item_ids(items, n_entity):
    x = items.long()
    return torch.where((x < 0) | (x > n_entity - 1), torch.full_like(x, n_entity - 1), x)


def clamp_words(ids, n):
    """32-bit words read unsigned and clamped to n - 1."""
    return (ids.long() & 0xFFFFFFFF).clamp(max=n - 1)


def clamp_users(users, n_user):
    return users.long().clamp(min=0, max=n_user - 1)


def _mem_lists(mem, users, n_user):
    """Per-hop lists [B, Nm] (long) of heads, relations, tails from either feed, ids as given."""
    if isinstance(mem, (tuple, list)):
        return tuple([t.long() for t in lst] for lst in mem)
    sel = mem[clamp_users(users, mem.shape[0] if n_user is None else n_user)].long()      # [B, P, 3, Nm]
    return tuple([sel[:, j, x] for j in range(sel.shape[1])] for x in range(3))


def small_reference(E, adj_e, adj_r, R, w_h, Wu, bu, t0, t1, W0, b0, W1, b1, W2, b2, A0, a0, A1, a1, Wmix, bmix, items, mem, users, P, K, nR,
                    depth=2, dtype=torch.float64, magnitude=False, parts=False):
    """``mem``: user_triplet_set [n_user, P, 3, Nm] (pair b reads users[b]'s sets) or the per-pair lists (mh, mr, mt); ``adj_r`` None:
    relations read as 0.  -> namespace(user_o [B, D], item_emb [B, D], scores [B], sigmoid [B]); with ``parts`` also o, logits, probs
    (keyaddr_reference's), nagg0, nagg1, out0, out1, out2 (out1 / out2 None at depth 1), child_rel, probs_parent, probs_child
    (l2_reference's; None without t0 or at depth 1)."""
    assert depth in (1, 2) and (W0 is None) == (W1 is None) and (depth == 1 or (W1 is None) == (W2 is None))
    n_entity, D = E.shape
    dev = E.device
    ab = (lambda t: t.abs()) if magnitude else (lambda t: t)
    f = lambda t: ab(t.to(dtype))                             # noqa: E731
    z = lambda t: 0 if t is None else f(t)                    # noqa: E731
    x = clamp_item_ids(items, n_entity)
    B = x.shape[0]
    mh, mr, mt = _mem_lists(mem, users, None)
    mh = [clamp_words(t, n_entity) for t in mh]
    mt = [clamp_words(t, n_entity) for t in mt]
    mr = [clamp_words(t, nR) for t in mr]
    ae = clamp_words(adj_e, n_entity)
    ar = clamp_words(adj_r, nR) if adj_r is not None else torch.zeros_like(ae)
    # ---- user side: the attention reads and the user MLP, logits as the kernel forms them (V = E[item] . R_KGE[r] first)
    ka = keyaddr_reference(E, R, w_h, None, None, (mh, mr, mt), None, x, P, dtype=dtype, order="vr_h")
    o = ka.o
    if magnitude:                                             # the weights of the true logits over absolute rows
        rows = ([mh[0]] if w_h is not None else []) + list(mt[:P])
        o = torch.stack([(p.to(dtype)[..., None] * f(E)[ids]).sum(1) for p, ids in zip(ka.probs, rows)], 1)
    user_o = o.reshape(B, -1) @ f(Wu) + z(bu)                 # model.py:232-236 (keyaddr_reference's own line; user_mlp_b may be absent)
    q = user_o
    # ---- the tree
    res = types.SimpleNamespace(user_o=user_o)
    if depth == 2:
        l2 = l2_reference(E, ae, ar, x, t0, t1, W1, W2, b1, b2, q if W1 is not None else None, A0, a0, B, 1, K, dtype=dtype,
                          magnitude=magnitude, parts=True)
        nagg0, nagg1, extra = l2[0], l2[1], l2[4]
        res.probs_parent, res.probs_child = l2[2], l2[3]
        if magnitude:
            ev0 = f(E)[x] if W0 is None else (f(E)[x] + q) @ f(W0) + z(b0)
            out0 = (ev0 + nagg0) @ f(A0) + z(a0)
            out2 = (out0 + nagg1) @ f(A1) + z(a1)
            item = torch.cat([ev0, out0, out2], 1) @ f(Wmix) + z(bmix)
            s = (user_o * item).sum(1)
            sg = torch.sigmoid(s)
            res.out0, res.out2, res.out1, res.child_rel = out0, out2, extra["out1"], extra["child_rel"]
        else:
            item, s, sg = tail_reference(E, x, q, user_o, nagg0, nagg1, W0, b0, A0, a0, A1, a1, Wmix, bmix, dtype=dtype)
        if parts and not magnitude:
            ev0 = f(E)[x] if W0 is None else (f(E)[x] + q) @ f(W0) + z(b0)
            res.out0 = torch.relu((ev0 + nagg0) @ f(A0) + z(a0))
            res.out2 = torch.relu((res.out0 + nagg1) @ f(A1) + z(a1))
            res.out1, res.child_rel = extra["out1"], extra["child_rel"]
    else:
        x1 = ae[x]                                            # [B, K]
        p0 = slot_weights(t0, ar[x], dtype)
        self1 = f(E)[x1] if W1 is None else (f(E)[x1] + q[:, None, :]) @ f(W1) + z(b1)
        nagg0 = (p0[..., None] * self1).sum(1) / K
        nagg1 = None
        ev0 = f(E)[x] if W0 is None else (f(E)[x] + q) @ f(W0) + z(b0)
        pre = (ev0 + nagg0) @ f(A0) + z(a0)
        out0 = pre if magnitude else torch.relu(pre)
        item = torch.cat([ev0, out0], 1) @ f(Wmix) + z(bmix)
        s = (user_o * item).sum(1)
        sg = torch.sigmoid(s)
        res.out0, res.out1, res.out2, res.child_rel, res.probs_parent, res.probs_child = out0, None, None, None, None, None
    res.item_emb, res.scores, res.sigmoid = item, s, sg
    if parts:
        res.o, res.logits, res.probs, res.nagg0, res.nagg1 = ka.o, ka.logits, ka.probs, nagg0, nagg1
        res.parent_rel = ar[x]
    return res
