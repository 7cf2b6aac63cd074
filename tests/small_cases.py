"""Worlds and cases of the single-launch pass (mvin_score_small_fwd) for tests/test_gpu_small_f64.py, with the conditions that keep a case
from passing vacuously; tests/test_small_ref_host.py checks those on the reference alone (TEST INFRASTRUCTURE).  Everything is drawn
with numpy generators seeded by the shape, so a world is the same on every device.

A REAL world joins the two sides the kernel joins:
    user side    keyaddr_ref.build_inputs(user_regime, ...): the entity table E, R_KGE, the h-set vector, the user MLP and the ripple sets
                 of N_USER users in one of keyaddr_ref.REGIMES; 256 pairs (keyaddr_ref.YARDSTICK_PAIRS), of which a case's are the first
    tree side    l2_cases.adjacency over the same entities (kinds counts / uniform), l2_cases.logits per tree regime, and W0 .. W2, A0,
                 A1, Wmix drawn N(0, 1 / D) with biases of 0.3 x the table's mean |component|: whatever the scale of the user regime's
                 table (0.1 .. 10), a pre-activation keeps the scale of its inputs, and the ReLUs pass about half of their elements
Pair i's item is l2_cases.parent_ids: entities (7 i) % K first -- every distinct-children count of the counts adjacency -- so the items
of the user-side draw are replaced (a planted world keeps its special entity out of them, as keyaddr_ref does).

An EXACT world holds small integers: entity rows in [-2, 2] at 25 % density (no all-zero row but the three ZERO entities at the end of
the table), every matrix four +-1 entries per column, biases in [-1, 1].  Its reads are ONE-HOT, planted as in keyaddr_ref: one user per
pair; every head of a row is a ZERO entity (logit exactly 0) except the planted slot (keyaddr_ref.planted_slot: it walks over the row with
the user index), whose head and relation are searched on the host so that its integer logit is positive; R_KGE and the h-set vector
carry a factor of 1024, so the planted logit leads by at least 1024 and every other weight is exactly 0 in fp32 AND in float64.  Tails
are distinct within a row: the o-vector names the slot.  Tree regimes none and planted (l2_cases).
"""
import functools
import types

import numpy as np
import torch

import keyaddr_ref as kr
import l2_cases as lc
from linear_valu_worker import ints, reals
from small_ref import small_reference

N_ENTITY = 603
N_USER = 37
N_ZERO = 3                                                    # exact worlds: entities n_entity - 3 .. n_entity - 1 have all-zero rows
OUTPUTS = ("user_o", "item_emb", "scores", "sigmoid")
BIASES = ("bu", "b0", "b1", "b2", "a0", "a1", "bmix")
LOGIT_FACTOR = 1024.0


def small_lds_bytes(D, G, K, nR, NO, Nm):
    """The LDS layout of mvin_score_small.hip (small_lds / small_lds_for), restated: words rounded up to 4 per array."""
    r4 = lambda n: (n + 3) & ~3                                # noqa: E731
    LD, nmt = D + 4, 16 if Nm <= 16 else 64
    njf = nmt * D // 256
    nparts = G * NO * (njf // 8 if njf > 8 else 1)
    head = 2 * r4(nR) + 2 * r4(G * LD) + r4(G * (NO * D + 4)) + r4(2 * G * D) + 32 + 7 * r4(G * K) + 2 * r4(16 * K)
    reads = r4(G * nR * D) + r4(nparts * (D + 4)) + r4(min(G, 4) * 3 * 4 * D)
    tree = 5 * r4(16 * LD) + r4((D // 16) * 16) + r4(16 * ((K + 7) // 8) * D)
    return 4 * (head + max(reads, tree))


def small_nr_limit(D, K, P, Nm):
    """The largest nR mvin_score_small_supported takes: one pair per workgroup, with the h-set read, within 160 KiB."""
    nR = 1
    while nR < 4096 and small_lds_bytes(D, 1, K, nR + 1, P + 1, Nm) <= 160 * 1024:
        nR += 1
    return nR


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _tree_side(w, rng, kind, exact):
    """Adjacency, the fields l2_cases.logits / conditions read, and the tree-side parameters."""
    D, K, n, nR, dev = w.D, w.K, w.n_entity, w.nR, w.device
    w.kind, w.exact, w.logits, w.refs, w.enc = kind, exact, {}, {}, None
    w.adj_e, w.adj_r = lc.adjacency(K, n - (N_ZERO if exact else 0), nR, kind, rng)
    if exact:                                                 # the zero entities have rows of their own and are nobody's neighbour
        extra_e, extra_r = lc.adjacency(K, n - N_ZERO, nR, kind, rng)
        w.adj_e, w.adj_r = np.concatenate([w.adj_e, extra_e[1:1 + N_ZERO]]), np.concatenate([w.adj_r, extra_r[1:1 + N_ZERO]])
    assert w.adj_e.shape == (n, K) and w.adj_e.min() >= 0 and w.adj_e.max() < n and w.adj_r.min() >= 0 and w.adj_r.max() < nR
    w.cnt = lc.distinct_slots(w.adj_e, w.adj_r, nR)
    w.ae, w.ar = _t(w.adj_e.astype(np.int32), dev), _t(w.adj_r.astype(np.int32), dev)
    if exact:
        mat = lambda rows=D: pm1(rng, rows, D, 4)             # noqa: E731
        vec = lambda: ints(rng, D, -1, 1)                     # noqa: E731
    else:
        s = float(w.E.abs().mean())
        mat = lambda rows=D: reals(rng, (rows, D), 1.0 / np.sqrt(D))      # noqa: E731
        vec = lambda: reals(rng, D, 0.3 * s)                  # noqa: E731
    for name in ("W0", "W1", "W2", "A0", "A1"):
        setattr(w, name, _t(mat(), dev))
    w.Wmix = _t(mat(3 * D), dev)
    for name in BIASES[1:]:
        setattr(w, name, _t(vec(), dev))
    return w


def pm1(rng, Din, Dout, nnz):
    """[Din, Dout] with nnz entries of +-1 per column."""
    W = np.zeros((Din, Dout), np.float32)
    for j in range(Dout):
        W[rng.choice(Din, min(nnz, Din), replace=False), j] = rng.choice([-1.0, 1.0], min(nnz, Din))
    return W


@functools.lru_cache(maxsize=None)
def world(D, K, Nm, P, nR, user_regime, kind, has_set, device, n_entity=N_ENTITY, n_user=N_USER, n_pairs=kr.YARDSTICK_PAIRS):
    """A real-valued world, built once and left unchanged."""
    inp = kr.build_inputs(user_regime, D, Nm, P, nR, n_pairs, n_user=n_user, n_entity=n_entity, has_set=has_set, device=device)
    rng = np.random.default_rng([D, K, Nm, P, nR, kr.REGIMES.index(user_regime), lc.KINDS.index(kind), int(has_set), 77])
    w = types.SimpleNamespace(D=D, K=K, Nm=Nm, P=P, nR=nR, n_entity=n_entity, n_user=inp.n_user, user_regime=user_regime, has_set=has_set,
                              device=device, inp=inp, N=inp.users.shape[0])
    w.E, w.R, w.w_h, w.Wu, w.bu, w.uts, w.users = inp.E, inp.R, inp.w, inp.W_mlp, inp.b_mlp, inp.uts, inp.users
    w.kind, w.n_entity = kind, n_entity
    items = lc.parent_ids(w, w.N)
    if inp.special is not None:
        items[items == inp.special] = (inp.special + 1) % n_entity
    w.items = inp.items = _t(items, device)
    # the tree-side parameters are redrawn until 30 % .. 70 % of out0, out1 and out2 pass their ReLU on 64 pairs, with and without
    # relation logits: the rows of the planted / ascending / descending / offset tables are all but parallel, so the sign of a column of
    # a pre-activation is nearly the same for every pair, and a draw can leave a ReLU almost shut or almost open
    for _ in range(50):
        _tree_side(w, rng, kind, False)
        shares = [float((getattr(r, name) > 0).double().mean()) for regime in ("unit", "none")
                  for r in [reference(make_case(w, regime, 64), n=64, parts=True)] for name in ("out0", "out1", "out2")]
        if 0.3 <= min(shares) and max(shares) <= 0.7:
            break
    else:
        raise AssertionError("no draw of the tree-side parameters keeps the ReLUs half open")
    # the combiner is scaled so that the scores have a root mean square of 3 (measured on the float64 reference of 64 pairs under the
    # unit tree regime): at the scale of the sharp / planted tables every sigmoid would be 0 or 1 in both precisions otherwise
    rms = float(reference(make_case(w, "unit", 64), n=64).scores.pow(2).mean().sqrt())
    w.Wmix, w.bmix = w.Wmix * (3.0 / rms), w.bmix * (3.0 / rms)
    return w


@functools.lru_cache(maxsize=None)
def exact_world(D, K, Nm, P, nR, tree_regime, has_set, device, n_entity=N_ENTITY, n_pairs=37):
    """An integer world with one-hot reads (the module's docstring), one user per pair."""
    assert tree_regime in lc.EXACT_REGIMES
    rng = np.random.default_rng([D, K, Nm, P, nR, lc.EXACT_REGIMES.index(tree_regime), int(has_set), 78])
    n, N = n_entity, n_pairs
    w = types.SimpleNamespace(D=D, K=K, Nm=Nm, P=P, nR=nR, n_entity=n, n_user=N, user_regime="planted-exact", has_set=has_set, device=device,
                              inp=None, N=N)
    E = ints(rng, (n, D), -2, 2) * (rng.random((n, D)) < 0.25)
    for e in np.flatnonzero(~E.any(1)):
        E[e, e % D] = 1.0
    E[n - N_ZERO:] = 0.0
    E = E.astype(np.float32)
    Ri = np.stack([pm1(rng, D, D, 4) for _ in range(nR)])
    wi = ints(rng, D, -1, 1)
    n_o = P + int(has_set)
    w.E = _t(E, device)
    _tree_side(w, rng, "planted" if tree_regime == "planted" else "counts", True)
    items = lc.parent_ids(w, N)
    uts = np.empty((N, P, 3, Nm), dtype=np.int32)
    uts[:, :, 0] = rng.integers(n - N_ZERO, n, (N, P, Nm))
    uts[:, :, 1] = rng.integers(0, nR, (N, P, Nm))
    for u in range(N):
        for j in range(P):
            uts[u, j, 2] = rng.choice(n - N_ZERO, Nm, replace=False)
            slot = kr.planted_slot(u, j, P, Nm)
            for _ in range(4000):
                r, a = int(rng.integers(0, nR)), int(rng.integers(0, n - N_ZERO))
                if (E[items[u]] @ Ri[r]) @ E[a] > 0 and (j > 0 or not has_set or E[a] @ wi > 0):
                    break
            else:
                raise AssertionError(f"exact world: no planted head for user {u}, hop {j}")
            uts[u, j, 0, slot], uts[u, j, 1, slot] = a, r
    w.R, w.w_h = _t((Ri * LOGIT_FACTOR).astype(np.float32), device), (_t((wi * LOGIT_FACTOR).astype(np.float32), device) if has_set else None)
    w.Wu, w.bu = _t(pm1(rng, n_o * D, D, 4), device), _t(ints(rng, D, -1, 1), device)
    w.uts, w.users, w.items = _t(uts, device), _t(np.arange(N, dtype=np.int64), device), _t(items, device)
    return w


def make_case(w, regime, B, depth=2, proj=True, null=(), adj_rel=True):
    """The first B pairs of the world under tree regime ``regime``; ``proj`` False: W0 .. W2 absent; ``null``: the biases passed as NULL;
    ``adj_rel`` False: no adj_relation (relations read as 0).  At depth 1 W2 / b2 / A1 / a1 / t1 are NULL, and the kernel is handed the
    whole [3D, D] Wmix, of which the contract reads the first 2 D rows."""
    assert B <= w.N and depth in (1, 2) and set(null) <= set(BIASES)
    c = types.SimpleNamespace(w=w, regime=regime, B=B, depth=depth, proj=proj, null=tuple(sorted(null)), adj_rel=adj_rel)
    c.t0, c.t1 = lc.logits(w, regime)
    a = dict(E=w.E, R=w.R, w_h=w.w_h, Wu=w.Wu, A0=w.A0, A1=w.A1, t0=c.t0, t1=c.t1)
    for name in ("W0", "W1", "W2"):
        a[name] = getattr(w, name) if proj else None
    for name in BIASES:
        a[name] = None if name in null else getattr(w, name)
    if depth == 1:
        a["W2"] = a["b2"] = a["A1"] = a["a1"] = a["t1"] = None
    c.a = a
    c.Wmix_ref = w.Wmix if depth == 2 else w.Wmix[:2 * w.D]
    c.parents_ext = w.items                                   # (l2_cases.conditions reads it)
    c.key = (regime, depth, proj, c.null, adj_rel)
    return c


def reference(c, dtype=torch.float64, n=None, items=None, uts=None, users=None, magnitude=False, parts=False, ar=None):
    """small_reference over the world's pairs (the first n), optionally with other ids."""
    w, a = c.w, c.a
    n = w.N if n is None else n
    ar = ar if ar is not None else (w.ar if c.adj_rel else None)
    return small_reference(a["E"], w.ae, ar, a["R"], a["w_h"], a["Wu"], a["bu"], a["t0"], a["t1"], a["W0"], a["b0"], a["W1"], a["b1"], a["W2"],
                           a["b2"], a["A0"], a["a0"], a["A1"], a["a1"], c.Wmix_ref, a["bmix"], (w.items if items is None else items)[:n],
                           w.uts if uts is None else uts, (w.users if users is None else users)[:n], w.P, w.K, w.nR, depth=c.depth, dtype=dtype,
                           magnitude=magnitude, parts=parts)


def references(c):
    """-> dict(r64: the float64 reference over all the world's pairs, with parts; yard: err_f32 per output over the same pairs;
    problems: the non-vacuity conditions missed), once per (world, case options)."""
    w = c.w
    if c.key not in w.refs:
        r64 = reference(c, parts=True)
        yard = None
        if not w.exact:
            r32 = reference(c, dtype=torch.float32)
            yard = {name: float((getattr(r32, name).double() - getattr(r64, name)).abs().max()) for name in OUTPUTS}
        w.refs[c.key] = dict(r64=r64, yard=yard, problems=conditions(c, r64))
    return w.refs[c.key]


def conditions(c, r):
    """On the float64 reference alone: the user-side regime is what it claims (keyaddr_ref.condition), the tree-side conditions of
    l2_cases.conditions (sharp rows, unit weights, probabilities summing to 1, every distinct-children count), and 20 % .. 80 % of
    out0, out1 and out2 pass their ReLU."""
    w, bad = c.w, []
    assert all(bool(torch.isfinite(getattr(r, n)).all()) for n in OUTPUTS)
    if w.inp is not None:
        try:
            kr.condition(w.inp, types.SimpleNamespace(logits=r.logits))
        except AssertionError as e:
            bad.append(f"user side ({w.user_regime}): {e}")
    else:                                                     # exact worlds: every read is one-hot on its planted slot
        for k, p in enumerate(r.probs):
            hop = max(0, k - int(w.has_set))
            want = torch.tensor([kr.planted_slot(u, hop, w.P, w.Nm) for u in range(p.shape[0])], device=p.device)
            if not (torch.equal(p.argmax(-1), want) and bool((p.max(-1).values == 1).all()) and bool((p.sum(-1) == 1).all())):
                bad.append(f"exact world: read {k} is not one-hot on its planted slot")
    for name in ("out0", "out1", "out2"):
        o = getattr(r, name)
        if o is not None:
            share = float((o > 0).double().mean())
            if not 0.2 <= share <= 0.8:
                bad.append(f"{share:.1%} of {name} pass the ReLU (20 % .. 80 % wanted)")
    if c.depth == 2 and c.adj_rel:
        probs = (None, None, r.probs_parent, r.probs_child)
        # (its ReLU share of out1 is the one above; a list of ONE slot has a weight of 1 in every regime)
        bad += [b for b in lc.conditions(c, probs, {"out1": r.out1, "child_rel": r.child_rel})
                if "out1" not in b and not (w.K == 1 and "in the unit regime" in b)]
    elif w.kind == "counts":
        missing = set(range(1, w.K + 1)) - set(w.cnt[w.items.cpu().numpy()].tolist())
        if missing:
            bad.append(f"distinct-children counts {sorted(missing)[:8]} do not occur among the parents")
    return bad


def exact_precondition(c, r64, outputs):
    """Magnitude x denominator < 2^24 for ``outputs`` and every intermediate they are made of, and the reference is a multiple of
    1 / K^2 (the aggregates' partial sums under planted weights 1 / m, m <= 4: 1 / (4 K^2)) -> list of what does not hold."""
    w, K, bad = c.w, c.w.K, []
    assert w.exact and c.regime in lc.EXACT_REGIMES
    mag = reference(c, magnitude=True, parts=True)
    inner = ("nagg0", "nagg1", "out0", "out2") if "item_emb" in outputs else ()
    for name in tuple(outputs) + inner:
        m, r = getattr(mag, name), getattr(r64, name)
        if m is None:
            continue
        # the planted weights 1 / m (m <= 4) sit on m EQUAL slots: only the partial sums over a list -- the aggregates -- see quarters;
        # a finished aggregate, and everything made of it, is a multiple of 1 / K^2
        denom = 4 * K * K if (c.regime == "planted" and name in ("nagg0", "nagg1")) else K * K
        if not float(m.max()) * denom < 2.0 ** 24:
            bad.append(f"{name}: magnitude {float(m.max()):.4g} x {denom} >= 2^24")
        if not bool((r.abs() <= m).all()):
            bad.append(f"{name}: magnitude below the value")
        if not torch.equal(r * (K * K), torch.round(r * (K * K))):
            bad.append(f"{name}: not a multiple of 1 / K^2")
    if not torch.equal(r64.user_o, torch.round(r64.user_o)):
        bad.append("user_o: not an integer (the reads are not one-hot)")
    return bad
