"""-m gpu: mvin_mf_head and mvin_mf_scores (ops.mf_head, ops.mf_scores) alone.

Cases: D in {4, 16, 64, 128} x G in {1 (BCE), 2, 5, 64} x n_groups in {1, 3, 257, 1000}, over tables of 7 users x 11 items
(every row shared many times) and of 1000 x 2000, both ranking modes at G >= 2; validity random at 80 %.

mf_head_kernel is compiled once per (L2, NP) -- 2^L2 lanes per row, NP passes over a group's rows (tests/rank_head_shapes.py
restates the rule) -- and that product reaches six of the twelve instances, with D / 4 always a power of two, so that no lane of
a row's lane group is ever without a chunk.  EXTRA (G, D), through the same checks, tables and n_groups, holds the rest:
  (3, 1)  (3, 20), (8, 24), (32, 32)    (3, 2)  (33, 32), (64, 24)    (4, 2)  (17, 36), (32, 64)
  (5, 2)  (9, 68), (16, 128)            (5, 4)  (17, 100), (32, 128)  -- D = 20, 24, 36, 68, 100: idle lanes (id loads, s_ok, the
          regulariser's sum); D = 32, 64, 128: none;
  (1, 1)  (4, 8), and (16, 64) at (4, 1): with 8 and 32 above, G a power of two in 4..32 (the segment of phase 2 is G lanes);
  BCE     (1, 20), (1, 32), (1, 100) at (3, 1), (3, 1), (5, 1).
G = 5 at D = 4, in the product, is the shape whose 408 slots take phase 2 through a second trip.  mvin_mf_scores runs at SCORES_DS: every
L2 of mf_scores_kernel, idle lanes at 12, 20 and 100.  Clamped ids and the integer tables run at (3, 20) and (17, 100) too: idle
lanes AND ids outside the tables.  tests/test_rank_head_shapes_host.py holds the lists to all that without a GPU.

Exact checks: scores and dscore equal mvin_gather_rows + mvin_rank_head bit for bit, du / di too at reg = 0, counts too; du / di
at reg != 0 equal the numpy float32 rule (mf_oracle.grad_rows32) applied to the device's OWN dscore; integer tables give exact
scores and an exact regulariser; masked slots are exactly 0 and a NaN label there reaches nothing; ids outside the tables are
clamped; guard words around every output are intact; a group's bits do not depend on n_groups, the grid, the launch or the
stream; mvin_mf_scores gives the head's logit bits.

Bounds against float64 (mf_oracle.head64), derived, with u = 2^-24:
  score    |err| <= delta = gamma_D * sum_k |u_k v_k|, gamma_D = D u / (1 - D u): D products and D - 1 adds in ANY order (the fmaf
           chain and the lane tree only round less often).
  dscore   |err| <= scale * (2 delta_g + 16 u), delta_g the largest delta among the group's valid slots.  Softmax: a logit error
           of at most delta_g moves exp(z_j - m) relatively by at most about delta_g twice (numerator and Z), and p_j <= 1;
           BPR: sigmoid' <= 1/4 on a difference of two scores, divided by |N_g|, and the positive's entry sums |N_g| such terms;
           BCE: sigmoid' <= 1/4.  16 u covers expf / log1pf (<= 2 ulp), the divisions, the subtraction and the <= 6 levels of a
           64-lane sum of terms that add up to at most 1.
  loss     |err| <= scale * (sum_g (2 delta_g + 16 u (1 + l_g)) + gamma_{n_groups} sum_g l_g): the same propagation into each
           group's loss (no term cancels: log Z >= 0 and m - z_0 >= 0; softplus >= 0), then a sum of n_groups terms in any
           order.
  BCE against mvin_eltwise mode 1 on the device's own scores: the dscore bound above.

Measured on the MI355X, worst error / bound:   score   dscore   loss
  the product GS x DS                          0.585   0.086    0.059
  the EXTRA shapes                             0.275   0.059    0.019
(the bounds are worst-case summation bounds, so a ratio well below 1 is what a correct kernel gives; the bit equalities are the
sharp checks, and they hold at every shape).
"""
import functools

import numpy as np
import pytest
import torch

import mf_oracle as mo

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DS = (4, 16, 64, 128)
GS = (1, 2, 5, 64)
NGROUPS = (1, 3, 257, 1000)
# (G, D) beside the product GS x DS: the smallest that reach what the product misses (tests/rank_head_shapes.py has the rule,
# tests/test_rank_head_shapes_host.py holds this list to it)
EXTRA = [(3, 20), (8, 24), (32, 32),          # (3, 1): idle lanes (5, 6 of 8 chunks) and full lanes; G a power of two
         (33, 32), (64, 24),                  # (3, 2)
         (17, 36), (32, 64),                  # (4, 2)
         (9, 68), (16, 128),                  # (5, 2)
         (17, 100), (32, 128),                # (5, 4)
         (4, 8), (16, 64),                    # (1, 1), which GS x DS has not; G a power of two at (1, 1) and (4, 1)
         (1, 20), (1, 32), (1, 100)]          # BCE at (3, 1) and (5, 1), with idle lanes and without
SHAPES = [(G, D) for G in GS for D in DS] + EXTRA
SCORES_DS = DS + (8, 12, 20, 32, 100)         # mvin_mf_scores: every L2, idle lanes at 12, 20 and 100
TABLES = ((7, 11), (1000, 2000))


def gamma(n):
    return n * U32 / (1.0 - n * U32)


@functools.lru_cache(maxsize=None)
def make_tables(n_user, n_item, D, integer=False):
    rng = np.random.default_rng(n_user * 131 + n_item * 7 + D)
    if integer:
        return (rng.integers(-3, 4, size=(n_user, D)).astype(np.float32), rng.integers(-3, 4, size=(n_item, D)).astype(np.float32))
    return (rng.normal(size=(n_user, D)).astype(np.float32), (1.5 * rng.normal(size=(n_item, D)) / np.sqrt(D)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def make_batch(n_user, n_item, n_groups, G):
    rng = np.random.default_rng(n_user + 13 * n_groups + 1000 * G)
    users = rng.integers(0, n_user, size=n_groups)
    items = rng.integers(0, n_item, size=n_groups * G)
    valid = (rng.random(n_groups * G) < 0.8).astype(np.float32)
    labels = (rng.random(n_groups * G) < 0.5).astype(np.float32)
    return users, items, valid, labels


def modes_of(G):
    return ("bce",) if G == 1 else ("bpr", "softmax")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


GUARD = -3.5


def run_head(U, V, users, items, mode, scale, reg, G, valid=None, labels=None, counts=True, grid_cap=0, stream=None):
    """ops.mf_head into guarded output buffers.  Returns a dict of numpy results; asserts the guard words."""
    from mvin_amd import ops
    B, D = len(items), U.shape[1]
    bufs = [torch.full((B + 2,), GUARD, device="cuda"), torch.full((B + 2,), GUARD, device="cuda"),
            torch.full((B + 2, D), GUARD, device="cuda"), torch.full((B + 2, D), GUARD, device="cuda")]
    acc = torch.zeros(4, device="cuda")
    acc[2:] = GUARD
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    cnt[2:] = -9
    args = (dev(U), dev(V), dev(users, torch.int64), dev(items, torch.int64), mode, scale, reg, acc[:2])
    kw = dict(group_size=G, valid=None if valid is None else dev(valid), labels=None if labels is None else dev(labels),
              counts=cnt[:2] if counts and mode != "bce" else None, out=tuple(b[1:-1] for b in bufs), grid_cap=grid_cap)
    torch.cuda.synchronize()
    if stream is None:
        ops.mf_head(*args, **kw)
    else:
        with torch.cuda.stream(stream):
            ops.mf_head(*args, **kw)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert (h[0] == GUARD).all() and (h[-1] == GUARD).all(), "a guard word around an output was written"
    acc, cnt = acc.cpu().numpy(), cnt.cpu().numpy()
    assert (acc[2:] == GUARD).all() and (cnt[2:] == -9).all()
    return dict(scores=host[0][1:-1], dscore=host[1][1:-1], du=host[2][1:-1], di=host[3][1:-1], loss=float(acc[0]),
                reg_loss=float(acc[1]), counts=tuple(int(c) for c in cnt[:2]))


def run_rank_head(U, V, users, items, mode, scale, G, valid):
    """The composition the head replaces: mvin_gather_rows x 2 + mvin_rank_head."""
    from mvin_amd import ops
    ur = ops.gather_rows(dev(U), dev(np.repeat(users, G), torch.int32))
    vr = ops.gather_rows(dev(V), dev(items, torch.int32))
    acc = torch.zeros(1, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = ops.rank_head(ur, vr, G, mode, scale, acc, valid=None if valid is None else dev(valid), counts=cnt)
    torch.cuda.synchronize()
    s, ds, du, di = (t.cpu().numpy() for t in out)
    return dict(scores=s, dscore=ds, du=du, di=di, counts=tuple(int(c) for c in cnt.cpu().numpy()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    bad = np.flatnonzero(bits(a).reshape(-1) != bits(b).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[0]}: {a.reshape(-1)[bad[0]]!r} != {b.reshape(-1)[bad[0]]!r}"


def bounds(U, V, users, items, G, val):
    """(delta [B], delta_g repeated over the group's rows [B])."""
    ur = np.repeat(np.abs(U[users].astype(np.float64)), G, axis=0)
    delta = gamma(U.shape[1]) * (ur * np.abs(V[items].astype(np.float64))).sum(axis=1)
    dg = np.where(val, delta, 0.0).reshape(-1, G).max(axis=1)
    return delta, np.repeat(dg, G)


def group_losses(ref, G, mode, scale):
    """The float64 per-group losses (unscaled), recomputed from the reference's scores."""
    s, val = ref["scores"].reshape(-1, G), ref["valid"].reshape(-1, G)
    out = np.zeros(s.shape[0])
    for g in range(s.shape[0]):
        if mode == "bce":
            continue
        w = val[g].copy()
        if mode == "softmax":
            z = s[g][w]
            out[g] = np.log(np.exp(z - z.max()).sum()) + z.max() - s[g, 0]
        else:
            w[0] = False
            if w.any():
                x = s[g][w] - s[g, 0]
                out[g] = (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).mean()
    return out


def check_head_shape(D, G, table):
    n_user, n_item = table
    U, V = make_tables(n_user, n_item, D)
    for n_groups in NGROUPS:
        users, items, valid, labels = make_batch(n_user, n_item, n_groups, G)
        scale, reg = 1.0 / n_groups, 0.07          # not a power of two: a product contracted into an fma would show
        for mode in modes_of(G):
            lab = None
            if mode == "bce":
                lab = labels.copy()
                lab[valid == 0] = np.nan                      # a masked row's label is never read
            got = run_head(U, V, users, items, mode, scale, 0.0, G, valid, lab)
            ref = mo.head64(U, V, users, items, mode, scale, 0.0, G, valid, labels)
            val = ref["valid"]
            # ---- exact: the composition of existing kernels
            if mode != "bce":
                comp = run_rank_head(U, V, users, items, mode, scale, G, valid)
                for k in ("scores", "dscore", "du", "di"):
                    same(got[k], comp[k], f"{k} against gather_rows + rank_head (D={D} G={G} n={n_groups} {mode})")
                assert got["counts"] == comp["counts"] == ref["counts"]
            else:
                assert got["counts"] == (0, 0)
            # ---- exact: masked slots
            assert not got["dscore"][~val].any() and not got["du"][~val].any() and not got["di"][~val].any()
            assert np.isfinite(got["dscore"]).all() and np.isfinite(got["loss"])
            # ---- float64 bounds
            delta, dg = bounds(U, V, users, items, G, val)
            e_s = np.abs(got["scores"] - ref["scores"])
            e_d = np.abs(got["dscore"] - ref["dscore"])
            print(f"D={D} G={G} n={n_groups} {mode}: score err/bound {float((e_s / delta).max()):.3f}, "
                  f"dscore err/bound {float((e_d / (scale * (2 * dg + 16 * U32))).max()):.3f}")
            assert (e_s <= delta).all()
            assert (e_d <= scale * (2 * dg + 16 * U32)).all()
            if mode == "bce":
                l = np.where(val, np.maximum(ref["scores"], 0) - ref["scores"] * labels + np.log1p(np.exp(-np.abs(ref["scores"]))), 0.0)
                lb = scale * ((2 * np.where(val, delta, 0) + 16 * U32 * (1 + l)).sum() + gamma(n_groups) * l.sum())
            else:
                l = group_losses(ref, G, mode, scale)
                lb = scale * ((2 * dg[::G] + 16 * U32 * (1 + l)).sum() + gamma(n_groups) * l.sum())
            print(f"    loss {got['loss']:.7g} ref {ref['loss']:.7g} err/bound {abs(got['loss'] - ref['loss']) / lb:.3f}")
            assert abs(got["loss"] - ref["loss"]) <= lb
            assert got["reg_loss"] == 0.0
            # ---- reg != 0: the bit rule from the device's own dscore; the regulariser within a summation bound
            gr = run_head(U, V, users, items, mode, scale, reg, G, valid, lab)
            same(gr["scores"], got["scores"], "scores with reg")
            same(gr["dscore"], got["dscore"], "dscore with reg")
            du, di = mo.grad_rows32(U, V, users, items, gr["dscore"], reg, G, val)
            same(gr["du"], du, f"du at reg != 0 (D={D} G={G} n={n_groups} {mode})")
            same(gr["di"], di, f"di at reg != 0 (D={D} G={G} n={n_groups} {mode})")
            refr = mo.head64(U, V, users, items, mode, scale, reg, G, valid, labels)
            assert abs(gr["reg_loss"] - refr["reg_loss"]) <= gamma(D * len(items) * 2 + 8) * refr["reg_loss"] + 1e-30


@pytest.mark.parametrize("table", TABLES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("D", DS)
def test_head_every_shape(D, G, table):
    check_head_shape(D, G, table)


@pytest.mark.parametrize("table", TABLES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("G,D", EXTRA)
def test_head_extra_shapes(G, D, table):
    """The instances, idle lanes and power-of-two groups that GS x DS does not reach, through every check of the product."""
    check_head_shape(D, G, table)


IDLE_AND_CLAMPED = [(3, 20), (17, 100)]       # a lane group wider than the row AND ids outside the tables


@pytest.mark.parametrize("G", GS)
def test_integer_tables_are_exact(G):
    check_integer_tables(G, 16)


@pytest.mark.parametrize("G,D", IDLE_AND_CLAMPED)
def test_integer_tables_are_exact_with_idle_lanes(G, D):
    check_integer_tables(G, D)


def check_integer_tables(G, D):
    U, V = make_tables(7, 11, D, integer=True)
    users, items, valid, labels = make_batch(7, 11, 257, G)
    for mode in modes_of(G):
        got = run_head(U, V, users, items, mode, 1.0, 0.5, G, valid, labels)
        ref = mo.head64(U, V, users, items, mode, 1.0, 0.5, G, valid, labels)
        assert np.array_equal(got["scores"].astype(np.float64), ref["scores"])
        assert got["reg_loss"] == ref["reg_loss"]                # integers below 2^24, reg / 2 a power of two
        if mode != "bce":
            assert got["counts"] == ref["counts"]                # exact ties occur (small integers) and count once


@pytest.mark.parametrize("D", DS)
def test_bce_against_eltwise(D):
    from mvin_amd import ops
    U, V = make_tables(1000, 2000, D)
    users, items, _, labels = make_batch(1000, 2000, 1000, 1)
    scale = 1.0 / 1000
    got = run_head(U, V, users, items, "bce", scale, 0.0, 1, None, labels)
    out, acc = torch.empty(1000, device="cuda"), torch.zeros(1, device="cuda")
    ops.eltwise(1, 1000, dev(got["scores"]), out, dev(labels), accum=acc, alpha=scale, beta=scale)
    delta, _ = bounds(U, V, users, items, 1, np.ones(1000, dtype=bool))
    assert (np.abs(out.cpu().numpy() - got["dscore"]) <= scale * (2 * delta + 16 * U32)).all()
    assert abs(float(acc.cpu()) - got["loss"]) <= scale * (2 * delta + 16 * U32 * 4).sum() + gamma(1000) * got["loss"]


@pytest.mark.parametrize("G", GS)
def test_ids_are_clamped(G):
    check_clamped_ids(G, 16)


@pytest.mark.parametrize("G,D", IDLE_AND_CLAMPED)
def test_ids_are_clamped_with_idle_lanes(G, D):
    check_clamped_ids(G, D)


def check_clamped_ids(G, D):
    n_user, n_item = 7, 11
    U, V = make_tables(n_user, n_item, D)
    users, items, valid, labels = make_batch(n_user, n_item, 257, G)
    users, items = users.copy(), items.copy()
    users[::5] = [-1, n_user, -(1 << 40), 1 << 40, n_user - 1, 0][G % 6]
    users[1::7] = -3
    items[::3] = n_item + 5
    items[1::4] = -2
    items[2::11] = 1 << 35
    for mode in modes_of(G):
        a = run_head(U, V, users, items, mode, 0.5, 0.25, G, valid, labels)
        b = run_head(U, V, np.clip(users, 0, n_user - 1), np.clip(items, 0, n_item - 1), mode, 0.5, 0.25, G, valid, labels)
        for k in ("scores", "dscore", "du", "di"):
            same(a[k], b[k], f"{k} with clamped ids")


@pytest.mark.parametrize("G,D", [(1, 64), (2, 4), (5, 64), (64, 128), (5, 16)])
def test_group_bits_do_not_depend_on_the_launch(G, D):
    """A group alone, among 1000 and under a forced small grid; a second launch and a second stream."""
    n_user, n_item = 1000, 2000
    U, V = make_tables(n_user, n_item, D)
    users, items, valid, labels = make_batch(n_user, n_item, 1000, G)
    for mode in modes_of(G):
        full = run_head(U, V, users, items, mode, 0.001, 0.125, G, valid, labels)
        for cap in (1, 3, 16):
            capped = run_head(U, V, users, items, mode, 0.001, 0.125, G, valid, labels, grid_cap=cap)
            for k in ("scores", "dscore", "du", "di"):
                same(capped[k], full[k], f"{k} under grid_cap={cap}")
            assert capped["counts"] == full["counts"]
        again = run_head(U, V, users, items, mode, 0.001, 0.125, G, valid, labels)
        other = run_head(U, V, users, items, mode, 0.001, 0.125, G, valid, labels, stream=torch.cuda.Stream())
        for k in ("scores", "dscore", "du", "di"):
            same(again[k], full[k], f"{k} of a second launch")
            same(other[k], full[k], f"{k} on a second stream")
        for g in (0, 1, 499, 999):
            rows = slice(g * G, g * G + G)
            alone = run_head(U, V, users[g:g + 1], items[rows], mode, 0.001, 0.125, G, valid[rows], labels[rows])
            for k in ("scores", "dscore", "du", "di"):
                same(alone[k], full[k][rows], f"{k} of group {g} alone")


@pytest.mark.parametrize("D", SCORES_DS)
def test_mf_scores_gives_the_head_bits(D):
    from mvin_amd import ops
    n_user, n_item = 1000, 2000
    U, V = make_tables(n_user, n_item, D)
    users, items, _, labels = make_batch(n_user, n_item, 1000, 1)
    users, items = users.copy(), items.copy()
    users[::9], items[::5] = -4, n_item + 1                      # clamped alike
    head = run_head(U, V, users, items, "bce", 1.0, 0.0, 1, None, labels)
    z, p = ops.mf_scores(dev(U), dev(V), dev(users, torch.int64), dev(items, torch.int64))
    same(z.cpu().numpy(), head["scores"], "mf_scores logits against the head's scores")
    zz = z.cpu().numpy().astype(np.float64)
    assert (np.abs(p.cpu().numpy() - 1.0 / (1.0 + np.exp(-zz))) <= 4 * U32).all()
    z1, none = ops.mf_scores(dev(U), dev(V), dev(users, torch.int64), dev(items, torch.int64), want_probs=False)
    none2, p1 = ops.mf_scores(dev(U), dev(V), dev(users, torch.int64), dev(items, torch.int64), want_logits=False)
    assert none is None and none2 is None
    same(z1.cpu().numpy(), head["scores"], "logits alone")
    same(p1.cpu().numpy(), p.cpu().numpy(), "probs alone")
    # the ranking layout: the head's rows are (user of the group, item of the row)
    users5, items5, _, _ = make_batch(n_user, n_item, 257, 5)
    h5 = run_head(U, V, users5, items5, "bpr", 1.0, 0.0, 5)
    z5, _ = ops.mf_scores(dev(U), dev(V), dev(np.repeat(users5, 5), torch.int64), dev(items5, torch.int64))
    same(z5.cpu().numpy(), h5["scores"], "mf_scores against the ranking head's scores")
