"""Worlds, logit regimes and cases of the fused two-level pass for tests/test_gpu_l2_f64.py, with the conditions that keep a case from
passing vacuously; tests/test_l2_ref_host.py checks those conditions on the reference alone (TEST INFRASTRUCTURE).  Everything is drawn
with numpy generators seeded by the shape, so a world is the same on every device.

Adjacency kinds (n_entity rows of K slots; every neighbour in [0, n_entity), every relation in [0, nR)):
    counts    row x holds x % K + 1 distinct (neighbour, relation) slots, the rest are repeats, shuffled: every distinct-children count
              1 .. K occurs as a parent and as a child
    uniform   K distinct neighbours per row: no repeats
    planted   relation 0 sits on m = 1, 2 or 4 slots of a row -- ONE (neighbour, 0) slot repeated m times -- every other slot has a
              relation >= 1: with the planted logits (t[0] = 0, the others in [-1000, -800]) every softmax weight is 0 or 1 / m
Row 0 is all zeros in every kind (one distinct slot of multiplicity K) and entity 0 is parent 0 of every case.  A row draws its
relations from a window of three (x, x + 1, x + 2 mod nR): rows then differ in their OWN largest logit, which is what the per-row
softmax forms exist for.

Logit regimes: unit (standard normal draws clipped to +-1.5: a spread of at most 3, no weight above 0.9 even at K = 4), sharp8 (8),
sharp130 (scale 130, redrawn until max - min > 60 on both tables and 15 % of all rows lie more than 60 below the maximum), offset
(unit + 1.0e4 rounded to fp32), none, t0, t1 (one table absent), planted.

Parents: parent i is entity (7 i) % K for i < K -- a bijection onto the counts 1 .. K of the counts world -- and (7 i) % n_entity
after that; parent i reads query row i // parents_per_pair.
"""
import functools
import types

import numpy as np
import torch

from l2_ref import l2_reference
from linear_valu_worker import ints, reals, to_bf16

N_ENTITY = 603
N_REL = 7
REAL_REGIMES = ("unit", "sharp8", "sharp130", "offset", "none", "t0", "t1")
EXACT_REGIMES = ("none", "planted")
KINDS = ("counts", "uniform", "planted")
# (table and bias range, weight range, non-zeros per weight column) of the exact cases by fan-out: the magnitudes shrink until
# magnitude x 4 K^2 < 2^24 (worst case out1: 819 at level 0, 146 at level 1, 21 at level 2)
EXACT_LEVELS = ((3, 2, 4), (2, 1, 4), (1, 1, 2))
MAX_QUERIES = 1024


def exact_level(K):
    return 0 if K <= 64 else 1 if K == 128 else 2


def sparse_ints(rng, Din, Dout, nnz, hi):
    """[Din, Dout] with at most nnz non-zeros in [-hi, hi] per column."""
    W = np.zeros((Din, Dout), np.float32)
    for j in range(Dout):
        W[rng.choice(Din, min(nnz, Din), replace=False), j] = rng.integers(-hi, hi + 1, min(nnz, Din))
    return W


def adjacency(K, n_entity, nR, kind, rng):
    """-> adj_e, adj_r int64 [n_entity, K]."""
    assert n_entity >= K and kind in KINDS and (kind != "planted" or nR >= 2)
    adj_e = np.zeros((n_entity, K), dtype=np.int64)
    adj_r = np.zeros((n_entity, K), dtype=np.int64)
    win = min(3, nR)
    for x in range(1, n_entity):
        if kind == "planted":
            m = min((1, 2, 4)[x % 3], K)
            rest = K - m
            e, r = [int(rng.integers(0, n_entity))] * m, [0] * m
            if rest:
                nd = (x // 3) % rest + 1
                ne = rng.choice(n_entity, nd, replace=False)
                nr = 1 + (x + rng.integers(0, win, nd)) % (nR - 1)
                pick = np.concatenate([np.arange(nd), rng.integers(0, nd, rest - nd)])
                e, r = np.concatenate([e, ne[pick]]), np.concatenate([r, nr[pick]])
            order = rng.permutation(K)
            adj_e[x], adj_r[x] = np.asarray(e)[order], np.asarray(r)[order]
            continue
        nd = x % K + 1 if kind == "counts" else K
        ne = rng.choice(n_entity, nd, replace=False)
        nr = (x + rng.integers(0, win, nd)) % nR
        pick = np.concatenate([np.arange(nd), rng.integers(0, nd, K - nd)])
        rng.shuffle(pick)
        adj_e[x], adj_r[x] = ne[pick], nr[pick]
    return adj_e, adj_r


def distinct_slots(adj_e, adj_r, nR):
    key = np.sort(adj_e * nR + adj_r, axis=1)
    return (np.diff(key, axis=1) != 0).sum(1) + 1


@functools.lru_cache(maxsize=None)
def world(D, K, n_entity, nR, kind, exact, device):
    """Tables, adjacency and parameters of one shape, built once and left unchanged."""
    rng = np.random.default_rng([D, K, n_entity, nR, KINDS.index(kind), int(exact)])
    adj_e, adj_r = adjacency(K, n_entity, nR, kind, rng)
    assert adj_e.min() >= 0 and adj_e.max() < n_entity and adj_r.min() >= 0 and adj_r.max() < nR      # the kernels index with these as they are
    w = types.SimpleNamespace(D=D, K=K, n_entity=n_entity, nR=nR, kind=kind, exact=exact, device=device)
    w.adj_e, w.adj_r, w.cnt = adj_e, adj_r, distinct_slots(adj_e, adj_r, nR)
    if exact:
        tv, wv, nnz = EXACT_LEVELS[exact_level(K)]
        val = lambda *s: ints(rng, s, -tv, tv)                # noqa: E731
        mat = lambda: sparse_ints(rng, D, D, nnz, wv)         # noqa: E731
    else:
        val = lambda *s: reals(rng, s, 0.3)                   # noqa: E731
        mat = lambda: reals(rng, (D, D), 0.3)                 # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    E = val(n_entity, D)
    w.E, w.E16 = t(E), t(to_bf16(E)).to(torch.bfloat16)
    w.ae, w.ar = t(adj_e.astype(np.int32)), t(adj_r.astype(np.int32))
    w.W1, w.W2, w.A0 = t(mat()), t(mat()), t(mat())
    w.b1, w.b2, w.a0 = t(val(D)), t(val(D)), t(val(D))
    w.q = t(val(MAX_QUERIES, D))
    w.logits, w.refs, w.enc, w.ws = {}, {}, None, {}
    return w


def _below(w, t, gap=60.0):
    """Share of all rows whose own largest logit lies more than ``gap`` below the table's."""
    return float((t[w.adj_r].max(1) < t.max() - gap).mean())


def logits(w, regime):
    """-> (t0, t1) fp32 tensors [nR] or None, drawn once per world and regime."""
    if regime in w.logits:
        return w.logits[regime]
    rng = np.random.default_rng([w.D, w.K, w.nR, sum(map(ord, regime))])
    nR = w.nR

    def draw():
        if regime in ("unit", "offset", "t0", "t1"):
            t = np.clip(reals(rng, nR), -1.5, 1.5)
            return (t + np.float32(1.0e4)).astype(np.float32) if regime == "offset" else t
        if regime == "sharp8":
            return reals(rng, nR, 8.0)
        if regime == "sharp130":
            for _ in range(1000):
                t = reals(rng, nR, 130.0)
                if nR == 1 or (t.max() - t.min() > 60 and _below(w, t) >= 0.15):
                    return t
            raise AssertionError("sharp130: no draw met its conditions")
        assert regime == "planted" and w.kind == "planted"
        return np.concatenate([[np.float32(0)], -rng.integers(800, 1001, nR - 1).astype(np.float32)])

    dev = lambda a: torch.from_numpy(a).to(w.device)          # noqa: E731
    t0 = None if regime in ("none", "t1") else dev(draw())
    t1 = None if regime in ("none", "t0") else dev(draw())
    w.logits[regime] = (t0, t1)
    return t0, t1


def parent_ids(w, n):
    i = np.arange(n, dtype=np.int64)
    return np.where(i < w.K, (7 * i) % w.K, (7 * i) % w.n_entity)


def make_case(w, regime, B, ppp=1, bias=True, proj=True, bf16=False, n_ref=None):
    """The case's P = B * ppp parents and B queries as the first of an extended set drawn the same way (at least ``n_ref`` parents:
    256, or K at K >= 128: every distinct-children count), over which the reference and the fp32 yardstick are taken."""
    P = B * ppp
    n_ref = n_ref or (w.K if w.K >= 128 else 256)
    Bx = -(-max(P, n_ref) // ppp)
    c = types.SimpleNamespace(w=w, regime=regime, B=B, ppp=ppp, P=P, bias=bias, proj=proj, bf16=bf16, Bx=Bx, Px=Bx * ppp)
    c.parents_ext = torch.from_numpy(parent_ids(w, c.Px)).to(w.device)
    c.t0, c.t1 = logits(w, regime)
    c.table = w.E16 if bf16 else w.E
    c.W1, c.W2 = (w.W1, w.W2) if proj else (None, None)
    c.b1, c.b2, c.a0 = (w.b1, w.b2, w.a0) if bias else (None, None, None)
    c.qx = w.q[:Bx] if Bx <= MAX_QUERIES else w.q[torch.arange(Bx, device=w.device) % MAX_QUERIES]      # pair b reads row b % 1024
    c.q = c.qx[:B]
    c.key = (regime, ppp, c.Px, bias, proj, bf16)
    return c


def reference(c, dtype=torch.float64, magnitude=False, parts=False):
    """l2_reference over the case's extended set."""
    w = c.w
    return l2_reference(c.table, w.ae, w.ar, c.parents_ext, c.t0, c.t1, c.W1, c.W2, c.b1, c.b2, c.qx, w.A0, c.a0, c.Bx, c.ppp, w.K,
                        dtype=dtype, magnitude=magnitude, parts=parts)


def references(c):
    """-> dict(r64, r32: the four outputs over the extended set; yard: err_f32 per output; problems: the non-vacuity conditions this
    case misses), computed once per (world, regime, parents, options)."""
    w = c.w
    if c.key not in w.refs:
        r = reference(c, parts=True)
        r64, extra = r[:4], r[4]
        r32 = reference(c, dtype=torch.float32)
        yard = [None if a is None else float((b.double() - a).abs().max()) for a, b in zip(r64, r32)]
        w.refs[c.key] = dict(r64=r64, r32=r32, yard=yard, problems=conditions(c, r64, extra))
    return w.refs[c.key]


def conditions(c, r64, extra):
    """The conditions that keep a case from passing vacuously, on the float64 reference alone -> list of the ones missed."""
    w, bad = c.w, []
    zeroed = float((extra["out1"] == 0).double().mean())
    if not 0.2 <= zeroed <= 0.8:
        bad.append(f"the ReLU zeroes {zeroed:.1%} of out1 (20 % .. 80 % wanted)")
    for name, p in (("probs_parent", r64[2]), ("probs_child", r64[3])):
        if p is not None:
            off = float((p.sum(-1) - 1).abs().max())
            if not off <= 1e-12:
                bad.append(f"{name} rows sum to 1 +- {off:.2e}")
            if c.regime in ("unit", "t0") and w.nR > 1 and float(p.max()) > 0.9:
                bad.append(f"{name}: a weight of {float(p.max()):.3f} in the unit regime")
    if c.regime == "sharp130" and w.nR > 1:
        for t in (c.t0, c.t1):
            if not float(t.max() - t.min()) > 60:
                bad.append("sharp130: a table with a spread of at most 60")
        own = c.t0[extra["child_rel"].long()].max(-1).values
        share = float((own < c.t0.max() - 60).double().mean())
        if share < 0.1:
            bad.append(f"sharp130: only {share:.1%} of the child rows lie more than 60 below the table's maximum")
    if w.kind == "counts":
        par = c.parents_ext.cpu().numpy()
        for who, rows in (("parents", par), ("children", w.adj_e[par].ravel())):
            missing = set(range(1, w.K + 1)) - set(w.cnt[rows].tolist())
            if missing:
                bad.append(f"distinct-children counts {sorted(missing)[:8]} do not occur among the {who}")
    if w.kind == "planted":
        m = (w.adj_r == 0).sum(1)
        if not ((m >= 1) & (m & (m - 1) == 0)).all():
            bad.append("planted: a row without a power-of-two number of planted slots")
        if not (distinct_slots(np.where(w.adj_r == 0, w.adj_e, -1), np.zeros_like(w.adj_r), 1) <= 2).all():
            bad.append("planted: the planted slots of a row are not one slot repeated")
    return bad


def exact_precondition(c, r64):
    """The exact cases' precondition, asserted on the reference: every partial sum is a multiple of 1 / (4 K^2) (1 / K^2 without planted
    weights of 1 / m, m <= 4) below 2^24 of them, and the results are multiples of 1 / K^2.  -> list of what does not hold."""
    w, K, bad = c.w, c.w.K, []
    assert w.exact and c.regime in EXACT_REGIMES
    denom = 4 * K * K if c.regime == "planted" else K * K
    mag = reference(c, magnitude=True)
    for name, r, m in zip(("nagg0", "nagg1"), r64, mag):
        if not float(m.max()) * denom < 2.0 ** 24:
            bad.append(f"{name}: magnitude {float(m.max()):.4g} x {denom} >= 2^24")
        if not bool((r.abs() <= m).all()):
            bad.append(f"{name}: magnitude below the value")
        if not torch.equal(r * (K * K), torch.round(r * (K * K))):
            bad.append(f"{name}: not a multiple of 1 / K^2")
    for name, p in (("probs_parent", r64[2]), ("probs_child", r64[3])):
        if p is not None and not bool(((p == 0) | (p == 1) | (p == 0.5) | (p == 0.25) | (p == 1.0 / K)).all()):
            bad.append(f"{name}: a weight that is not 0 or 1 / m")
    if c.proj:                                               # the projected-tables forms multiply E . W1 . A0 (and E . W2 . A0) first
        d = lambda t: t.double().abs()                        # noqa: E731
        tab = max(float((d(c.table) @ d(w.W1) @ d(w.A0)).max()), float((d(c.table) @ d(w.W2) @ d(w.A0)).max()))
        if not tab * denom < 2.0 ** 24:
            bad.append(f"projected tables: magnitude {tab:.4g} x {denom} >= 2^24")
    return bad
