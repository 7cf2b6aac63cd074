"""-m gpu: mvin_sparse_adam_rows (ops.sparse_adam_rows) alone, BIT FOR BIT against the numpy float32 restatement of its rule
(tests/mf_oracle.py: adam_rows32 -- stable run order, left-to-right sums, every operation rounded on its own).

n in {1, 2, 63, 64, 65, 4097} x D in {4, 8, 32, 64, 128} x n_rows in {1, 5, 1000}, and D in {12, 20, 100} -- where 1, 3 and 7
lanes of a row's lane group hold no chunk of the row -- at n in {1, 65, 4097} only (a reduction, to keep the module's time down:
the run structure does not depend on D, and those three n are one lane group, more than one workgroup (64, 32 and 8 lane groups each), and
the long launch).  D covers every instance of the kernel: sparse_adam_rows_kernel<L2>, L2 = 0, 1, 2, 3, 3, 4, 5, 5 for the eight dims
(tests/rank_head_shapes.py; tests/test_rank_head_shapes_host.py holds DS to it).  The one run of 4097 and the grid caps run at
D = 20 and 32 too (L2 = 3, with idle lanes and without).  Keys distinct / all equal (one run of 4097) /
geometric run lengths / random; runs masked whole, a masked first entry, valid absent; keys below 0 and at n_rows, order words
outside [0, n); zero, huge, denormal and NaN gradients; every grid cap; a second launch and a second stream.  All three tables
sit between guard rows, and every byte of tables and guards is compared, so a row outside the runs that moved shows.
On the MI355X every case of every dim equals the rule bit for bit (the check has no tolerance, so there is no ratio to record).
"""
import numpy as np
import pytest
import torch

import mf_oracle as mo

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 4097)
DS = (4, 8, 12, 20, 32, 64, 100, 128)        # every L2 of the kernel (0, 1, 2, 3, 3, 4, 5, 5); idle lanes at 12, 20 and 100
IDLE_DS = (12, 20, 100)                      # a lane group wider than the row: 3 of 4, 5 of 8, 25 of 32 lanes hold a chunk
IDLE_NS = (1, 65, 4097)
ROWS = (1, 5, 1000)
CASES = [(n, D, n_rows) for n_rows in ROWS for D in DS for n in (IDLE_NS if D in IDLE_DS else NS)]
HP = (np.float32(0.0123), np.float32(0.9), np.float32(0.999), np.float32(1e-8))
GUARD = np.float32(-7.25)


def tables(n_rows, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_rows, D)).astype(np.float32)
    m = (0.1 * rng.normal(size=(n_rows, D))).astype(np.float32)
    v = (0.01 * rng.random(size=(n_rows, D))).astype(np.float32)
    return x, m, v


def make_keys(kind, n, n_rows, rng):
    if kind == "distinct":
        return rng.permutation(n_rows)[:n].astype(np.int64)
    if kind == "equal":
        return np.full(n, n_rows // 2, dtype=np.int64)
    if kind == "geometric":                    # runs of 1, 2, 4, ... entries, shuffled in place
        keys, k, run = [], 0, 1
        while len(keys) < n:
            keys += [k % n_rows] * run
            k, run = k + 1, run * 2
        return rng.permutation(np.array(keys[:n], dtype=np.int64))
    return rng.integers(0, n_rows, size=n).astype(np.int64)


def run_device(x, m, v, keys, grads, valid, order=None, grid_cap=0, stream=None, hp=HP):
    """The call on guarded copies of the tables.  Returns (x, m, v with their guard rows, status)."""
    from mvin_amd import ops
    dev = torch.device("cuda")
    big = []
    for t in (x, m, v):
        b = np.full((t.shape[0] + 2, t.shape[1]), GUARD, dtype=np.float32)
        b[1:-1] = t
        big.append(torch.from_numpy(b).to(dev))
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    args = (torch.from_numpy(np.asarray(keys, dtype=np.int64)).to(dev), torch.from_numpy(grads).to(dev))
    kw = dict(valid=None if valid is None else torch.from_numpy(valid).to(dev),
              order=None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).to(dev), grid_cap=grid_cap)
    torch.cuda.synchronize()
    if stream is None:
        ops.sparse_adam_rows(big[0][1:-1], big[1][1:-1], big[2][1:-1], *args, *[float(h) for h in hp], status, **kw)
    else:
        with torch.cuda.stream(stream):
            ops.sparse_adam_rows(big[0][1:-1], big[1][1:-1], big[2][1:-1], *args, *[float(h) for h in hp], status, **kw)
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in big] + [tuple(status.cpu().tolist())]


def expect(x, m, v, keys, grads, valid, order=None, hp=HP):
    x, m, v = x.copy(), m.copy(), v.copy()
    st = mo.adam_rows32(x, m, v, keys, grads, valid, *hp, order=order)
    out = []
    for t in (x, m, v):
        b = np.full((t.shape[0] + 2, t.shape[1]), GUARD, dtype=np.float32)
        b[1:-1] = t
        out.append(b)
    return out + [st]


def same_bits(got, ref):
    for name, g, r in zip("xmv", got[:3], ref[:3]):
        bad = np.argwhere((g.view(np.uint32) != r.view(np.uint32)) & ~(np.isnan(g) & np.isnan(r)))      # any NaN equals any NaN
        assert bad.size == 0, f"{name}: {len(bad)} words differ, first at row {bad[0][0] - 1} col {bad[0][1]}: " \
                              f"{g[tuple(bad[0])]!r} != {r[tuple(bad[0])]!r}"
    assert got[3] == ref[3], f"status {got[3]} != {ref[3]}"


def check(x, m, v, keys, grads, valid, **kw):
    hp = kw.get("hp", HP)
    got = run_device(x, m, v, keys, grads, valid, **kw)
    same_bits(got, expect(x, m, v, keys, grads, valid, order=kw.get("order"), hp=hp))
    return got


@pytest.mark.parametrize("n,D,n_rows", CASES)
def test_bits_every_shape(n, D, n_rows):
    """Every (n, D, n_rows) of CASES: random keys with a random mask, then the same keys without a mask; distinct keys where they fit."""
    rng = np.random.default_rng(1000 * n + 10 * D + n_rows)
    x, m, v = tables(n_rows, D, n + D)
    grads = rng.normal(size=(n, D)).astype(np.float32)
    keys = make_keys("random", n, n_rows, rng)
    valid = (rng.random(n) < 0.7).astype(np.float32)
    got = check(x, m, v, keys, grads, valid)
    assert got[3][0] == len(np.unique(keys[valid != 0])) and got[3][1] == 0
    check(x, m, v, keys, grads, None)
    if n <= n_rows:
        got = check(x, m, v, make_keys("distinct", n, n_rows, rng), grads, None)
        assert got[3] == (n, 0)


@pytest.mark.parametrize("D", (4, 20, 32, 64, 128))
def test_one_run_of_4097_and_geometric_runs(D):
    rng = np.random.default_rng(D)
    n, n_rows = 4097, 1000
    x, m, v = tables(n_rows, D, 5)
    grads = rng.normal(size=(n, D)).astype(np.float32)
    got = check(x, m, v, make_keys("equal", n, n_rows, rng), grads, None)
    assert got[3] == (1, 0)
    valid = (rng.random(n) < 0.5).astype(np.float32)
    check(x, m, v, make_keys("equal", n, n_rows, rng), grads, valid)
    keys = make_keys("geometric", n, n_rows, rng)
    got = check(x, m, v, keys, grads, valid)
    assert got[3][0] == len(np.unique(keys[valid != 0]))


def test_masked_runs_and_masked_first_entry():
    rng = np.random.default_rng(11)
    n, n_rows, D = 65, 5, 64
    x, m, v = tables(n_rows, D, 6)
    grads = rng.normal(size=(n, D)).astype(np.float32)
    keys = make_keys("random", n, n_rows, rng)
    valid = np.ones(n, dtype=np.float32)
    valid[keys == 3] = 0                                  # a run masked whole: row 3 keeps x, m AND v
    valid[np.flatnonzero(keys == 1)[0]] = 0               # the first entry of a run masked: the sum starts at the second
    valid[np.flatnonzero(keys == 2)[:5]] = 0
    got = check(x, m, v, keys, grads, valid)
    for t, t0 in zip(got[:3], (x, m, v)):
        assert np.array_equal(t[1 + 3], t0[3])
    assert got[3] == (4, 0)
    got = check(x, m, v, keys, grads, np.zeros(n, dtype=np.float32))
    assert got[3] == (0, 0)


def test_keys_and_order_words_out_of_range_are_dropped_and_counted():
    rng = np.random.default_rng(12)
    n, n_rows, D = 200, 5, 16
    x, m, v = tables(n_rows, D, 7)
    grads = rng.normal(size=(n, D)).astype(np.float32)
    keys = make_keys("random", n, n_rows, rng)
    bad = rng.permutation(n)[:30]
    keys[bad] = np.array([-1, -5, n_rows, n_rows + 7, -(1 << 40), 1 << 40] * 5)
    got = check(x, m, v, keys, grads, None)
    assert got[3] == (n_rows, 30)
    order = np.argsort(keys, kind="stable").astype(np.int64)
    for at, word in ((0, -1), (50, n), (51, 1 << 30), (120, -(1 << 31)), (n - 1, n + 5)):
        order[at] = word                                  # dropped as if absent: the runs around them stay whole
    got = check(x, m, v, keys, grads, (rng.random(n) < 0.8).astype(np.float32), order=order)
    assert got[3][1] >= 5


def test_special_values():
    """v = 0 with g = 0 (0 / eps); a huge gradient (g * g overflows: v = inf and the step is 0); denormal gradients; a NaN
    gradient and an overflowing sum (inf / inf) stay inside their rows.  A NaN's payload is not part of the rule."""
    n_rows, D = 6, 8
    x, m, v = tables(n_rows, D, 8)
    v[0] = 0
    m[0, :4] = 0
    keys = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], dtype=np.int64)
    g = np.zeros((10, D), dtype=np.float32)
    g[2] = 3e38
    g[4], g[5] = 1e-40, -3e-41
    g[6, 3] = np.nan
    g[7] = 1.0
    g[8], g[9] = 3e38, 3e38                               # the sum overflows: m' = v' = inf
    got = check(x, m, v, keys, g, None)
    assert got[3] == (5, 0)
    gx = got[0][1:-1]
    nan = np.isnan(gx)
    assert nan[3, 3] and nan[4].all() and nan.sum() == 1 + D
    assert np.array_equal(gx[0, :4], x[0, :4])            # m' = 0, v' = 0: the step is 0 / eps = 0
    assert np.array_equal(gx[1], x[1]) and np.isinf(got[2][1:-1][1]).all()
    assert np.array_equal(gx[5], x[5])


@pytest.mark.parametrize("cap", (1, 2, 3, 7, 64))
def test_bits_do_not_depend_on_the_grid(cap):
    for D in (64, 20, 32):                                # L2 = 4; L2 = 3 with idle lanes and without
        rng = np.random.default_rng(13)
        n, n_rows = 4097, 1000
        x, m, v = tables(n_rows, D, 9)
        grads = rng.normal(size=(n, D)).astype(np.float32)
        keys = make_keys("geometric", n, n_rows, rng)
        valid = (rng.random(n) < 0.9).astype(np.float32)
        check(x, m, v, keys, grads, valid, grid_cap=cap)


def test_second_launch_and_second_stream():
    rng = np.random.default_rng(14)
    n, n_rows, D = 4097, 1000, 128
    x, m, v = tables(n_rows, D, 10)
    grads = rng.normal(size=(n, D)).astype(np.float32)
    keys = make_keys("random", n, n_rows, rng)
    a = check(x, m, v, keys, grads, None)
    b = run_device(x, m, v, keys, grads, None)
    c = run_device(x, m, v, keys, grads, None, stream=torch.cuda.Stream())
    same_bits(b, a)
    same_bits(c, a)
    # an order from another stable sort gives the same bits: they depend on (x, m, v, keys, grads, valid) alone
    same_bits(run_device(x, m, v, keys, grads, None, order=np.argsort(keys, kind="stable")), a)
