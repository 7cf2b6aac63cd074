"""-m gpu: mvin_resample_sums against tests/resample_oracle.py.  Integer-valued tables (any summation order is exact) bit for bit
against a plain integer computation over the oracle's draws; real-valued tables bit for bit against the order-mimicking oracle and
within gamma_U sum|x| of math.fsum; NaN cells, a whole-NaN column, infinities; strided rows; a column's bits alone and among
others; replicate splitting; every workgroup cap; the observed mode; two seeds.  Every output is guarded."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_oracle as ro
from mvin_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
PATTERN = 0x5A5A5A5A
MODES = ("bootstrap", "signflip", "observed")
ROWS = (0, 1, 63, 64, 65, 129, 4097)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype):
    words = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
    whole = torch.full((words + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    return whole[GUARD:GUARD + words].view(dtype).view(shape), whole


def intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == PATTERN).all() and (w[-GUARD:] == PATTERN).all())


def run(vals, n_rep, mode, seed=1, first=0, max_groups=0, ld=None):
    """One guarded ops.resample_sums call on a host table (``ld``: rows that many doubles apart): (sums, counts) on the host."""
    n_rows, n_cols = vals.shape
    if ld is None:
        t = dev(vals)
    else:
        buf = np.full((n_rows, ld), 1.0e300)                        # what lies between the rows must not be read
        buf[:, :n_cols] = vals
        t = dev(buf)[:, :n_cols]
    (s, ws), (c, wc) = guarded((n_rep, n_cols), torch.float64), guarded((n_rep, n_cols), torch.int32)
    got = ops.resample_sums(t, n_rep, seed=seed, mode=mode, first=first, max_groups=max_groups, out=(s, c))
    torch.cuda.synchronize()
    assert got[0] is s and got[1] is c
    assert intact(ws) and intact(wc), "a write outside an output buffer"
    return s.cpu().numpy(), c.cpu().numpy()


def col_counts():
    cap = ops.resample_max_cols()
    assert cap >= 16
    return (1, 3, 8, cap, cap + 5)


def real_table(n_rows, n_cols, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_rows, n_cols)) * 10.0 ** rng.integers(-3, 4, (n_rows, n_cols))


@pytest.mark.parametrize("n_rows", ROWS)
def test_integer_tables_are_exact(hip_lib, n_rows):
    rng = np.random.default_rng(n_rows)
    for n_cols in col_counts():
        iv = rng.integers(-(1 << 20), (1 << 20) + 1, (n_rows, n_cols))
        for mode in MODES:
            for n_rep in (1, 5):
                s, c = run(iv.astype(np.float64), n_rep, mode, seed=3)
                rows, signs = ro.draws(mode, 3, n_rows, range(n_rep))
                want = (iv[rows] * signs.astype(np.int64)[:, :, None]).sum(axis=1)
                assert (s == want.astype(np.float64)).all() and not np.signbit(s[s == 0]).any(), (n_cols, mode, n_rep)
                assert (c == n_rows).all()


@pytest.mark.parametrize("n_rows", [r for r in ROWS if r])
def test_real_tables_match_the_oracle_bit_for_bit(hip_lib, n_rows):
    for n_cols in col_counts():
        v = real_table(n_rows, n_cols, 100 + n_cols)
        for mode in MODES:
            s, c = run(v, 5, mode, seed=7)
            ws, wc = ro.resample_sums(v, mode, 7, range(5))
            assert ro.same_bits(s, ws) and (c == wc).all(), (n_cols, mode)
            # three columns only: math.fsum is a Python loop (host time); every column is pinned bit for bit above
            f, fc, fa = ro.resample_fsum(v[:, :3], mode, 7, range(5))
            assert (np.abs(s[:, :3] - f) <= ro.gamma(n_rows) * fa).all() and (c[:, :3] == fc).all()


def test_three_hundred_replicates(hip_lib):
    v = real_table(129, 8, 5)
    for mode in ("bootstrap", "signflip"):
        s, c = run(v, 300, mode, seed=11)
        ws, wc = ro.resample_sums(v, mode, 11, range(300))
        assert ro.same_bits(s, ws) and (c == wc).all()
        assert len({x.tobytes() for x in s}) > 290                 # the replicates differ


def test_nan_cells_a_nan_column_and_infinities(hip_lib):
    rng = np.random.default_rng(8)
    v = real_table(200, 6, 9)
    v[rng.random(200) < 0.3, 0] = np.nan
    v[:, 1] = np.nan                                               # a whole-NaN column: count 0, sum +0.0
    v[rng.random(200) < 0.05, 2] = np.inf
    v[rng.random(200) < 0.05, 3] = -np.inf
    v[5, 4], v[77, 4] = np.inf, -np.inf                            # inf - inf wherever both are drawn: some NaN
    for mode in MODES:
        s, c = run(v, 40, mode, seed=2)
        ws, wc = ro.resample_sums(v, mode, 2, range(40))
        assert ro.same_bits(s, ws) and (c == wc).all(), mode
        assert (c[:, 1] == 0).all() and (s[:, 1].view(np.uint64) == 0).all()
        assert (c[:, 0] < 200).all() and (c[:, 5] == 200).all()
        if mode != "signflip":
            assert np.isposinf(s[:, 2]).any() and not np.isnan(s[:, 2]).any() and np.isneginf(s[:, 3]).any()
    assert np.isnan(run(v, 1, "observed")[0][0, 4])


def test_strided_rows(hip_lib):
    v = real_table(130, 5, 21)
    for mode in MODES:
        dense = run(v, 6, mode, seed=4)
        for ld in (6, 7, 16):                                      # even and odd: both load widths
            got = run(v, 6, mode, seed=4, ld=ld)
            assert ro.same_bits(got[0], dense[0]) and (got[1] == dense[1]).all(), (mode, ld)


def test_a_column_alone_and_among_others(hip_lib):
    cap = ops.resample_max_cols()
    v = real_table(257, cap + 5, 33)
    v[::9, 2] = np.nan
    for mode in MODES:
        s, c = run(v, 7, mode, seed=6)
        for col in (0, 2, 7, cap - 1, cap, cap + 4):
            a = run(v[:, col:col + 1], 7, mode, seed=6)
            assert ro.same_bits(a[0][:, 0], s[:, col]) and (a[1][:, 0] == c[:, col]).all(), (mode, col)
        b = run(v[:, 1:4], 7, mode, seed=6)                        # another width, another alignment of the rows
        assert ro.same_bits(b[0], s[:, 1:4]) and (b[1] == c[:, 1:4]).all()


def test_replicate_splitting(hip_lib):
    v = real_table(300, 4, 12)
    for mode in ("bootstrap", "signflip"):
        whole = run(v, 10, mode, seed=5)
        part = run(v, 4, mode, seed=5, first=3)
        assert ro.same_bits(part[0], whole[0][3:7]) and (part[1] == whole[1][3:7]).all()
        far = run(v, 2, mode, seed=5, first=(1 << 40) + 1)
        want = ro.resample_sums(v, mode, 5, [(1 << 40) + 1, (1 << 40) + 2])
        assert ro.same_bits(far[0], want[0])


def test_workgroup_cap_changes_no_bit(hip_lib):
    v = real_table(500, 9, 14)
    for mode in MODES:
        base = run(v, 37, mode, seed=8, max_groups=0)
        for g in (1, 3):
            got = run(v, 37, mode, seed=8, max_groups=g)
            assert ro.same_bits(got[0], base[0]) and (got[1] == base[1]).all(), (mode, g)


def test_observed_ignores_seed_and_replicate(hip_lib):
    v = real_table(4097, 3, 15)
    a = run(v, 3, "observed", seed=1)
    b = run(v, 3, "observed", seed=99, first=17)
    want = ro.resample_sums(v, "observed", 0, [0])
    for r in range(3):
        assert ro.same_bits(a[0][r], want[0][0]) and ro.same_bits(b[0][r], want[0][0])
    assert (a[1] == 4097).all() and (b[1] == 4097).all()


def test_two_seeds_differ(hip_lib):
    v = real_table(100, 2, 16)
    for mode in ("bootstrap", "signflip"):
        a, b = run(v, 8, mode, seed=1), run(v, 8, mode, seed=2)
        assert (a[0] != b[0]).all()
        again = run(v, 8, mode, seed=1)
        assert ro.same_bits(a[0], again[0])


def test_nothing_to_do_and_refusals_launch_nothing(hip_lib):
    from mvin_amd import _lib
    v = real_table(10, 3, 17)
    s, c = run(v, 0, "bootstrap")
    assert s.shape == (0, 3) and c.shape == (0, 3)
    s, c = run(np.zeros((0, 4)), 3, "bootstrap")
    assert (s.view(np.uint64) == 0).all() and (c == 0).all()
    s, c = run(np.zeros((5, 0)), 3, "signflip")
    assert s.shape == (3, 0)
    # refused calls leave guarded outputs untouched
    t = dev(v)
    (so, ws), (co, wc) = guarded((4, 3), torch.float64), guarded((4, 3), torch.int32)
    p = lambda x: C.c_void_p(x.data_ptr())                         # noqa: E731
    cap = hip_lib.mvin_resample_max_cols()
    for args in ((p(t), 10, 3, 3, 3, 1, 0, 4, 0, p(so), p(co)), (p(t), -1, 3, 3, 0, 1, 0, 4, 0, p(so), p(co)),
                 (p(t), 10, 3, 2, 0, 1, 0, 4, 0, p(so), p(co)), (p(t), 10, cap + 1, cap + 1, 0, 1, 0, 4, 0, p(so), p(co)),
                 (p(t), 10, 3, 3, 0, 1, -1, 4, 0, p(so), p(co)), (None, 10, 3, 3, 0, 1, 0, 4, 0, p(so), p(co))):
        assert hip_lib.mvin_resample_sums(*args, None) < 0
    torch.cuda.synchronize()
    inner = torch.cat([so.reshape(-1).view(torch.int32), co.reshape(-1)]).cpu().numpy()
    assert (inner == PATTERN).all() and intact(ws) and intact(wc)
    with pytest.raises(ValueError):
        ops.resample_sums(t, 3, mode="jackknife")
    with pytest.raises(ValueError):
        ops.resample_sums(t, -1)
    with pytest.raises(ValueError):
        ops.resample_sums(t.t(), 3)                                # columns not dense
    with pytest.raises(TypeError):
        ops.resample_sums(t.float(), 3)
    with pytest.raises(_lib.MvinHipError):
        ops.resample_sums(t.cpu(), 3)
