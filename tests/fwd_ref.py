"""Float64 statements of the contracts of the per-level forward kernels (mvin_amd/csrc/mvin_kernels.hip and
mvin_linear_mfma.hip), written from the comments in include/mvin_hip.h, not from the kernels' loops (TEST INFRASTRUCTURE).

Same conventions as tests/bwd_ref.py, whose ``precision`` switch, ``staged_x``, ``strided`` and ``softmax`` are used here and
not copied: numpy in, float64 out (or the dtype of ``precision``), and ``magnitude=True`` returns for every output the sum of
the ABSOLUTE values of the terms that make it up (softmax weights stay what they are; a ReLU is left out: it is 1-Lipschitz, so
the bound of its argument holds for it).  tests/test_fwd_ref_host.py pins every function to an independent torch float64
statement of the same formula; tests/test_gpu_fwd_kernels.py compares the kernels with them.

bf16 tables: the caller passes the values the table holds (already rounded to bf16), as float32; the arithmetic is fp32 on the
device and float64 here either way.
"""
import numpy as np

import bwd_ref
from bwd_ref import precision, softmax, staged_x, strided  # noqa: F401  (precision is this module's switch too)


def _f(x):
    return bwd_ref._f(x)


def _ids(i):
    return np.asarray(i).astype(np.int64)


# ----------------------------------------------------------------------------------------------- mvin_linear_fwd
def linear(srcs, W, Dout, *, rows, ids=None, bias=None, rowbias=None, rows_per_group=1, relu=False, sum_sources=False,
           nz=1, w_zstride=0, bias_zstride=0, src_rows=0, score_u=None, out=None, out_offset=0, ldo=None, out_zstride=0,
           magnitude=False):
    """out[z][r, :] = act(concat_s(X_s[r, :]) . W[z] + bias[z] + rowbias[r // rows_per_group, :]).
    X_s[r] = src[s][r] or src[s][ids[s][r]]; a gathered id outside [0, src_rows) reads row src_rows - 1 (src_rows = 0: no
    clamp); sum_sources: X = sum_s X_s.  W = None: identity copy.  W / bias are flat buffers, slab z at z * zstride.
    score[r] = sum_j out[r, j] * score_u[r, j], sigmoid[r] = 1 / (1 + exp(-score[r])) (nz == 1).
    ``out`` (a flat pre-filled buffer) given: also returns ``flat``, that buffer with out[z][r, j] stored at
    out_offset + z * out_zstride + r * ldo + j and nothing else touched.
    Returns dict(out [nz, rows, Dout], score [rows] | None, sigmoid [rows] | None, flat | None)."""
    ab = np.abs if magnitude else (lambda a: a)
    nsrc = len(srcs)
    ids = list(ids) if ids is not None else [None] * nsrc
    if src_rows > 0:
        ids = [None if i is None else np.where((_ids(i) < 0) | (_ids(i) >= src_rows), src_rows - 1, _ids(i)) for i in ids]
    X = staged_x([ab(_f(s)) for s in srcs], ids, sum_sources, rows)
    Din = X.shape[1]
    res = np.zeros((nz, rows, Dout), X.dtype)
    for z in range(nz):
        if W is None:
            assert Din == Dout and (nsrc == 1 or sum_sources)
            y = X.copy()
        else:
            y = X @ ab(_f(np.asarray(W).ravel()[z * w_zstride:z * w_zstride + Din * Dout].reshape(Din, Dout)))
        if bias is not None:
            y = y + ab(_f(np.asarray(bias).ravel()[z * bias_zstride:z * bias_zstride + Dout]))
        if rowbias is not None:
            y = y + ab(_f(rowbias).reshape(-1, Dout))[np.arange(rows) // rows_per_group]
        if relu and not magnitude:
            y = np.maximum(y, 0)
        res[z] = y
    ret = {"out": res, "score": None, "sigmoid": None, "flat": None}
    if score_u is not None:
        assert nz == 1, "the score epilogue of a z-batched call is not defined"
        ret["score"] = (res[0] * ab(_f(score_u).reshape(rows, Dout))).sum(axis=1)
        with np.errstate(over="ignore"):           # exp(-score) = inf gives the right limit, 0
            ret["sigmoid"] = 1.0 / (1.0 + np.exp(-ret["score"]))
    if out is not None:
        ldo = ldo or Dout
        flat = _f(out).ravel().copy()
        for z in range(nz):
            idx = out_offset + z * out_zstride + np.arange(rows)[:, None] * ldo + np.arange(Dout)[None, :]
            flat[idx] = res[z]
        ret["flat"] = flat
    return ret


# ----------------------------------------------------------------------------------------------- aggregator
def agg(self_vec, Wagg, bagg, K, *, child=None, rel_ids=None, table=None, adj_entity=None, adj_relation=None,
        node_ids=None, rel_score=None, Wc=None, c_child=None, N=1, magnitude=False):
    """mvin_agg_fwd_ex (dense: child [T*K, D], rel_ids [T*K] | None) and mvin_gather_attn_fwd_ex (gather: children are
    table[adj_entity[node_ids[t], k]], relations adj_relation[node_ids[t], k]) for node task t = b * N + n:
        p   = softmax_k(rel_score[r_k])  (no rel_score: p_k = 1;  dense with rel_ids None: rel_score is one logit per child)
        S   = sum_k p_k child_k
        agg = (S . Wc + (sum_k p_k) c_child[b]) / K   (no Wc: S / K;  no c_child: that term is absent)
        Z   = self_vec[t] + agg ;  out[t] = relu(Z . Wagg + bagg)
    Returns dict(out [T, D], probs [T, K] | None, S [T, D] = S / K (the kernel's s_out), Z [T, D])."""
    ab = np.abs if magnitude else (lambda a: a)
    sv = ab(_f(self_vec))
    T, D = sv.shape
    if table is not None:
        x = _ids(node_ids)[:T]
        c = ab(_f(table))[_ids(adj_entity).reshape(-1, K)[x]]                               # [T, K, D]
        rel = _ids(adj_relation).reshape(-1, K)[x] if rel_score is not None else None
    else:
        c = ab(_f(child)).reshape(T, K, D)
        rel = _ids(rel_ids).reshape(T, K) if rel_ids is not None else None
    if rel_score is None:
        p, probs = np.ones((T, K), sv.dtype), None
    else:
        p = softmax(_f(rel_score)[rel] if rel is not None else _f(rel_score).reshape(T, K))
        probs = p
    S = np.einsum("tk,tkd->td", p, c)
    if Wc is not None:
        a = S @ ab(_f(Wc))
        if c_child is not None:
            a = a + p.sum(axis=1, keepdims=True) * ab(_f(c_child))[np.arange(T) // N]
    else:
        a = S
    Z = sv + a / K
    out = Z @ ab(_f(Wagg))
    if bagg is not None:
        out = out + ab(_f(bagg))
    if not magnitude:
        out = np.maximum(out, 0)
    return {"out": out, "probs": probs, "S": S / K, "Z": Z}


# ----------------------------------------------------------------------------------------------- ripple-set read
def ripple_attn(E, score_ids, value_ids, mode, *, rel_ids=None, V=None, w=None, nR=None, magnitude=False):
    """mode 0: s_m = E[score_ids[b, m]] . V[b, rel_ids[b, m], :];  mode 1: s_m = E[score_ids[b, m]] . w[0:D];
    o[b, :] = sum_m softmax_m(s)_m E[value_ids[b, m], :].  Returns dict(o [B, D], probs [B, Nm], logits [B, Nm])."""
    E = _f(E)
    D = E.shape[1]
    sid, vid = _ids(score_ids), _ids(value_ids)
    B = sid.shape[0]
    h = E[sid]
    if mode == 0:
        v = _f(V).reshape(B, nR, D)[np.arange(B)[:, None], _ids(rel_ids)]
        s = np.einsum("bmd,bmd->bm", h, v)
    else:
        s = h @ _f(w).ravel()[:D]
    p = softmax(s)
    t = np.abs(E[vid]) if magnitude else E[vid]
    return {"o": np.einsum("bm,bmd->bd", p, t), "probs": p, "logits": s}


# ----------------------------------------------------------------------------------------------- small kernels
def rel_score(relation_emb, urh_weights, magnitude=False):
    """t[r] = relation_emb[r, :] . urh_weights[D:2D]."""
    rel, w = _f(relation_emb), _f(urh_weights).ravel()
    if magnitude:
        rel, w = np.abs(rel), np.abs(w)
    D = rel.shape[1]
    return rel @ w[D:2 * D]


def expand_ids(adj_entity, adj_relation, items, K, levels, n_entity):
    """entities[0] = items clamped to [0, n_entity - 1]; entities[e + 1][b, j * K + k] = adj_entity[entities[e][b, j], k];
    relations[e][b, j * K + k] = adj_relation[entities[e][b, j], k].  Returns (entities [levels + 1], relations [levels])."""
    ents = [np.clip(_ids(items), 0, n_entity - 1).reshape(-1, 1)]
    rels = []
    for _ in range(levels):
        p = ents[-1]
        ents.append(_ids(adj_entity).reshape(-1, K)[p].reshape(p.shape[0], -1))
        rels.append(_ids(adj_relation).reshape(-1, K)[p].reshape(p.shape[0], -1))
    return ents, rels
