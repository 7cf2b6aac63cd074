"""Float64 statements of the contracts of the training kernels (mvin_amd/csrc/mvin_bwd.hip), written from the comments
in include/mvin_hip.h and above each kernel, not from the kernels' loops (TEST INFRASTRUCTURE).

Every function takes numpy arrays, computes in float64 and returns what the kernel ADDS to its (caller-zeroed or
pre-filled) outputs.  tests/test_bwd_ref_host.py pins each of them to torch.autograd on the forward formula it is the
backward of; tests/test_gpu_bwd_kernels.py compares the kernels with them.

``magnitude=True`` returns, for every output, the sum of the ABSOLUTE values of the terms that make it up (inputs
replaced by their absolute values, differences by sums; softmax weights and masks stay what they are).  Two uses:
  * exact integer cases: every partial sum of the kernel, in whatever order, is a multiple of 1/denominator bounded by
    that magnitude, so magnitude * denominator < 2^24 means float32 holds all of them exactly;
  * real-valued sum-of-products cases: the worst case of any-order float32 summation of n float32 products is
    (n + 2) * 2^-24 * magnitude.
"""
import contextlib

import numpy as np
import torch

F64 = np.float64
_DT = F64


@contextlib.contextmanager
def precision(dtype):
    """Evaluate the formulas in another precision (float32: how much of a tolerance the FORMULA itself uses up when it
    is evaluated in the kernels' number format -- the real-valued GPU cases assert that this stays small)."""
    global _DT
    old, _DT = _DT, np.dtype(dtype).type
    try:
        yield
    finally:
        _DT = old


def _f(x):
    return np.asarray(x, dtype=_DT)


def _index_add(n_rows, ids, rows):
    """out[ids[i], :] += rows[i, :] (torch's index_add_: np.add.at is far too slow at 10^5 rows)."""
    rows = np.ascontiguousarray(rows, dtype=_DT)
    out = torch.zeros((n_rows,) + rows.shape[1:], dtype=torch.from_numpy(np.zeros(0, _DT)).dtype)
    out.index_add_(0, torch.from_numpy(np.asarray(ids).astype(np.int64).ravel()), torch.from_numpy(rows))
    return out.numpy()


def softmax(x, axis=-1):
    x = _f(x)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


# ----------------------------------------------------------------------------------------------- weight gradient
def staged_x(srcs, ids=None, sum_sources=False, rows=None):
    """X as mvin_linear_fwd stages it: source s is src[s][ids[s][r], :] (or src[s][r, :] without ids); the sources are
    concatenated along the columns, or summed."""
    ids = ids or [None] * len(srcs)
    parts = []
    for s, i in zip(srcs, ids):
        s = _f(s).reshape(-1, np.asarray(s).shape[-1])
        parts.append(s[np.asarray(i).astype(np.int64).ravel()[:rows]] if i is not None else s[:rows])
    return sum(parts[1:], parts[0]) if sum_sources else np.concatenate(parts, axis=1)


def strided(flat, z, zstride, rows, ld, cols):
    """[rows, cols] view of slab z of a flat buffer with row stride ld and slab stride zstride."""
    flat = np.asarray(flat).ravel()
    idx = z * zstride + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    return flat[idx]


def wgrad(srcs, dY, Dout, *, ids=None, sum_sources=False, mask=None, rows, nz=1, ldy=None, dy_zstride=0, ldm=None,
          mask_zstride=0, magnitude=False):
    """dW[z] = X^T . (dY[z] where mask[z] > 0), db[z] = its column sums.  dY / mask: flat buffers addressed as
    [z * zstride + r * ld + j].  Returns (dW [nz, Din, Dout], db [nz, Dout])."""
    ldy, ldm = ldy or Dout, ldm or Dout
    X = staged_x(srcs, ids, sum_sources, rows)
    if magnitude:
        X = staged_x([np.abs(_f(s)) for s in srcs], ids, sum_sources, rows)
    dW = np.zeros((nz, X.shape[1], Dout), _DT)
    db = np.zeros((nz, Dout), _DT)
    for z in range(nz):
        G = _f(strided(dY, z, dy_zstride, rows, ldy, Dout))
        if magnitude:
            G = np.abs(G)
        if mask is not None:
            G = np.where(strided(mask, z, mask_zstride, rows, ldm, Dout) > 0, G, 0.0)
        dW[z] = X.T @ G
        db[z] = G.sum(axis=0)
    return dW, db


# ----------------------------------------------------------------------------------------------- neighbor mix
def agg_bwd(dvec, K, nR, *, child=None, rel_ids=None, table=None, adj_entity=None, adj_relation=None, node_ids=None,
            probs=None, rel_score=None, magnitude=False):
    """Backward of agg[t] = (1/K) sum_k p[t,k] c[t,k] given dvec = dL/d agg (T rows).
    Children: dense (child [T*K, D], rel_ids [T*K]) or rows of ``table`` through the adjacency of node x = node_ids[t]
    (x = t without node_ids: the by-entity form).  Weights: ``probs`` [T, K] as given, softmax_k(rel_score[rel]) or,
    with neither, all ones (no attention: a plain mean, no dT).
        g_k = dvec . c_k ;  dc_k = (p_k / K) dvec ;  dlogit_k = (p_k / K) (g_k - sum_j p_j g_j)
    Returns dict(dchild [T*K, D] | dtable [n_rows, D], dT [nR] | None)."""
    dvec = _f(dvec)
    T, D = dvec.shape
    gather = table is not None
    if gather:
        x = np.arange(T) if node_ids is None else np.asarray(node_ids).astype(np.int64)[:T]
        ce = np.asarray(adj_entity).astype(np.int64).reshape(-1, K)[x]                    # [T, K] child rows
        rel = np.asarray(adj_relation).astype(np.int64).reshape(-1, K)[x] if adj_relation is not None else None
        c = _f(table)[ce]                                                                 # [T, K, D]
    else:
        c = _f(child).reshape(T, K, D)
        rel = np.asarray(rel_ids).astype(np.int64).reshape(T, K) if rel_ids is not None else None
    att = probs is not None or rel_score is not None
    if probs is not None:
        p = _f(probs).reshape(T, K)
    elif rel_score is not None:
        p = softmax(_f(rel_score)[rel])
    else:
        p = np.ones((T, K), _DT)
    sgn = -1.0
    if magnitude:
        dvec, c, sgn = np.abs(dvec), np.abs(c), 1.0
    g = np.einsum("td,tkd->tk", dvec, c)
    pg = (p * g).sum(axis=1, keepdims=True)
    dc = (p / K)[:, :, None] * dvec[:, None, :]
    out = {"dT": None}
    if att:
        dl = (p / K) * (g + sgn * pg)
        out["dT"] = np.bincount(rel.ravel(), weights=dl.ravel(), minlength=nR)[:nR]
    if gather:
        out["dtable"] = _index_add(np.asarray(table).shape[0], ce, dc.reshape(T * K, D))
    else:
        out["dchild"] = dc.reshape(T * K, D)
    return out


def rel_score_bwd(relation_emb, urh_weights, dT, magnitude=False):
    """Backward of t[r] = Rel[r] . w[D:2D]: drel[r, :] = dT[r] w[D:2D]; durh[D:2D] = sum_r dT[r] Rel[r, :] (the rest
    of durh [3D] receives nothing).  Returns (drel [nR, D], durh [3D])."""
    rel, w, dT = _f(relation_emb), _f(urh_weights).ravel(), _f(dT).ravel()
    if magnitude:
        rel, w, dT = np.abs(rel), np.abs(w), np.abs(dT)
    D = rel.shape[1]
    durh = np.zeros(w.shape[0], _DT)
    durh[D:2 * D] = dT @ rel
    return dT[:, None] * w[None, D:2 * D], durh


# ----------------------------------------------------------------------------------------------- key addressing
def key_addressing_fwd(E, V, w, mem_h, mem_r, mem_t, P, nR):
    """out [B, (w given) + P, D]: slot 0 (w given) = sum_m softmax_m(E[h0_m] . w) E[h0_m]; then per hop
    sum_m softmax_m(E[h_m] . V[b, r_m]) E[t_m]."""
    E = _f(E)
    B = np.asarray(mem_h[0]).shape[0]
    outs = []
    if w is not None:
        h0 = E[np.asarray(mem_h[0]).astype(np.int64)]
        outs.append(np.einsum("bm,bmd->bd", softmax(h0 @ _f(w).ravel()), h0))
    Vv = _f(V).reshape(B, nR, -1) if P > 0 else None
    for hop in range(P):
        h, t = E[np.asarray(mem_h[hop]).astype(np.int64)], E[np.asarray(mem_t[hop]).astype(np.int64)]
        v = Vv[np.arange(B)[:, None], np.asarray(mem_r[hop]).astype(np.int64)]
        outs.append(np.einsum("bm,bmd->bd", softmax(np.einsum("bmd,bmd->bm", h, v)), t))
    return np.stack(outs, axis=1)


def key_addressing_bwd(E, V, w, mem_h, mem_r, mem_t, P, dout, ldo, nR, l2, *, relation_kge=None, items=None,
                       magnitude=False):
    """Backward of key_addressing_fwd plus the regulariser l2 * sum over hops, pairs, memories of (|E[h]|^2 + |E[t]|^2):
      hop : do = dout[b, slot] ; g_m = do . t_m ; dl_m = p_m (g_m - sum p g)
            dE[t_m] += p_m do + 2 l2 t_m ; dE[h_m] += dl_m V[b, r_m] + 2 l2 h_m ; dV[b, r_m] += dl_m h_m
      set : ds = dout[b, 0]  ; g'_m = ds . h0_m ; dl'_m = p'_m (g'_m - sum p' g')
            dE[h0_m] += p'_m ds + dl'_m w ;  dw += dl'_m h0_m
      item share (relation_kge [nR, D, D] and items [B] given; V[b, r, :] = E[item_b] . R[r]):
            dE[item_b, i] += sum_r sum_j dV[b, r, j] R[r, i, j]
    dout is a flat buffer, row stride ldo, slot s at columns [s D, (s + 1) D).
    Returns dict(dE [nE, D], dV [B, nR, D] | None, dw [D] | None, reg)."""
    Er = _f(E)
    nE, D = Er.shape
    B, Nm = np.asarray(mem_h[0]).shape
    slot0 = 1 if w is not None else 0
    do_all = _f(strided(dout, 0, 0, B, ldo, (slot0 + P) * D)).reshape(B, slot0 + P, D)
    Ea = np.abs(Er) if magnitude else Er
    sgn = 1.0 if magnitude else -1.0
    if magnitude:
        do_all = np.abs(do_all)
    dE = np.zeros((nE, D), _DT)
    out = {"dV": None, "dw": None, "reg": _DT(0.0)}
    bi = np.arange(B)[:, None]
    if w is not None:
        wr = _f(w).ravel()
        ih = np.asarray(mem_h[0]).astype(np.int64)
        p = softmax(Er[ih] @ wr)
        h0, ds, wa = Ea[ih], do_all[:, 0], (np.abs(wr) if magnitude else wr)
        g = np.einsum("bd,bmd->bm", ds, h0)
        dl = p * (g + sgn * (p * g).sum(axis=1, keepdims=True))
        dE += _index_add(nE, ih, (p[:, :, None] * ds[:, None, :] + dl[:, :, None] * wa).reshape(-1, D))
        out["dw"] = np.einsum("bm,bmd->d", dl, h0)
    if P > 0:
        Vr = _f(V).reshape(B, nR, D)
        Va = np.abs(Vr) if magnitude else Vr
        dV = np.zeros((B, nR, D), _DT)
        for hop in range(P):
            ih, it = np.asarray(mem_h[hop]).astype(np.int64), np.asarray(mem_t[hop]).astype(np.int64)
            ir = np.asarray(mem_r[hop]).astype(np.int64)
            p = softmax(np.einsum("bmd,bmd->bm", Er[ih], Vr[bi, ir]))
            h, t, v, do = Ea[ih], Ea[it], Va[bi, ir], do_all[:, slot0 + hop]
            g = np.einsum("bd,bmd->bm", do, t)
            dl = p * (g + sgn * (p * g).sum(axis=1, keepdims=True))
            dE += _index_add(nE, it, (p[:, :, None] * do[:, None, :] + 2 * l2 * t).reshape(-1, D))
            dE += _index_add(nE, ih, (dl[:, :, None] * v + 2 * l2 * h).reshape(-1, D))
            dV += _index_add(B * nR, (bi * nR + ir), (dl[:, :, None] * h).reshape(-1, D)).reshape(B, nR, D)
            out["reg"] += l2 * ((h * h).sum() + (t * t).sum())
        out["dV"] = dV
        if relation_kge is not None:
            R = _f(relation_kge).reshape(nR, D, D)
            if magnitude:
                R = np.abs(R)
            dE += _index_add(nE, np.asarray(items).astype(np.int64), np.einsum("brj,rij->bi", dV, R))
    out["dE"] = dE
    return out


# ----------------------------------------------------------------------------------------------- small kernels
def scatter_add_rows(n_rows, ids, x, alpha=1.0, magnitude=False):
    """dtable[ids[r], :] += alpha x[r, :]."""
    x = _f(x)
    return _index_add(n_rows, ids, (abs(alpha) * np.abs(x)) if magnitude else alpha * x)


def count_ids(ids, nbins):
    """out[b] += |{i : ids[i] == b}| for 0 <= b < nbins; other ids are ignored."""
    ids = np.asarray(ids).astype(np.int64).ravel()
    ids = ids[(ids >= 0) & (ids < nbins)]
    return np.bincount(ids, minlength=nbins).astype(_DT)


def eltwise(mode, x, y=None, z=None, w=None, alpha=1.0, beta=0.0, beta1=0.0, beta2=0.0, eps=0.0, D=1, N=1,
            magnitude=False):
    """The mvin_eltwise family (include/mvin_hip.h).  Returns dict with the arrays the mode writes (y; for mode 4: x,
    z = m, w = v) and ``accum``, the amount added to *accum (modes 1, 3, 7, 8)."""
    x = _f(x).ravel()
    ab = np.abs if magnitude else (lambda a: a)
    if mode == 0:
        return {"y": ab(alpha) * ab(x) + (ab(beta) * ab(_f(y).ravel()) if beta != 0 else 0.0)}
    if mode == 1:      # tf.nn.sigmoid_cross_entropy_with_logits and its gradient
        lab = _f(z).ravel()
        ce = np.maximum(x, 0) - x * lab + np.log1p(np.exp(-np.abs(x)))
        return {"y": (1.0 / (1.0 + np.exp(-x)) - lab) * alpha, "accum": beta * ce.sum()}
    if mode == 2:
        return {"y": np.where(_f(z).ravel() > 0, ab(x), 0.0)}
    if mode == 3:
        return {"accum": ab(alpha) * (x * x).sum()}
    if mode == 4:      # Adam: x param, y grad, z m, w v, alpha = lr_t
        g = _f(y).ravel()
        m = beta1 * _f(z).ravel() + (1 - beta1) * g
        v = beta2 * _f(w).ravel() + (1 - beta2) * g * g
        return {"x": x - alpha * m / (np.sqrt(v) + eps), "z": m, "w": v}
    if mode == 5:
        X = x.reshape(-1, D)
        out = ab(alpha) * ab(_f(z).ravel()[:X.shape[0], None]) * ab(X)
        if beta != 0:
            out = out + ab(beta) * ab(_f(y).ravel().reshape(-1, D))
        return {"y": out.ravel()}
    if mode == 6:
        return {"y": (ab(alpha) * ab(x.reshape(-1, N, D)).sum(axis=1)).ravel()}
    if mode == 7:
        X = x.reshape(-1, D)
        return {"accum": ab(alpha) * (ab(_f(z).ravel()[:X.shape[0]]) * (X * X).sum(axis=1)).sum()}
    if mode == 8:      # x is the TABLE, z the int32 row ids
        X = x.reshape(-1, D)[np.asarray(z).astype(np.int64).ravel()]
        return {"accum": ab(alpha) * (X * X).sum()}
    raise ValueError(mode)


def l2_adam(xs, l2s, g, m=None, v=None, *, apply_adam=False, lr_t=0.0, beta1=0.9, beta2=0.999, eps=1e-8,
            magnitude=False):
    """mvin_l2_adam_multi over the segments xs[s] (coefficient l2s[s]) laid end to end in the flat buffers g, m, v:
        g += c x ; loss += (c / 2) sum x^2 ; then (apply_adam) m, v, x <- Adam(g, lr_t).
    Returns dict(xs: list, g, m, v, loss)."""
    flat = np.concatenate([_f(a).ravel() for a in xs])
    c = np.concatenate([np.full(np.asarray(a).size, float(l), _DT) for a, l in zip(xs, l2s)])
    g = _f(g).ravel()[:flat.size]
    if magnitude:
        flat, g, c = np.abs(flat), np.abs(g), np.abs(c)
    g = g + c * flat
    out = {"loss": (0.5 * c * flat * flat).sum(), "g": g, "m": None, "v": None}
    if apply_adam:
        out["m"] = beta1 * _f(m).ravel()[:flat.size] + (1 - beta1) * g
        out["v"] = beta2 * _f(v).ravel()[:flat.size] + (1 - beta2) * g * g
        flat = flat - lr_t * out["m"] / (np.sqrt(out["v"]) + eps)
    offs = np.cumsum([0] + [np.asarray(a).size for a in xs])
    out["xs"] = [flat[offs[i]:offs[i + 1]].reshape(np.asarray(a).shape) for i, a in enumerate(xs)]
    return out
