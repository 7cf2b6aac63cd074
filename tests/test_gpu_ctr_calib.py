"""-m gpu: mvin_ctr_calib / ops.ctr_calib against the float64 oracle: the integer columns bit for bit, the eight sums within the
summation bound of tests/ctr_calib_oracle.py, the confidence mass within two units a pair, and the same bits on every launch and
for every ``max_groups``."""
import numpy as np
import pytest
import torch

from ctr_calib_oracle import calib_oracle_rows, platt_targets, sum_bound
from mvin_amd import ops

pytestmark = pytest.mark.gpu

SEG_LENS = [1, 63, 64, 65, 255, 256, 257, 4096, 4097]        # a chunk is 4 096 pairs
MAPS = [(1.0, 0.0), (0.125, -0.5), (3.0, 2.0)]


def _edges(n_bins):
    """Ascending z-edges that contain 0 and values the logits below take."""
    if n_bins == 1:
        return np.zeros(0, np.float32)
    if n_bins == 2:
        return np.zeros(1, np.float32)
    if n_bins == 10:
        return np.arange(-4, 5).astype(np.float32)
    return (np.arange(63) / 8 - 31 / 8).astype(np.float32)


def _run(z, y, a=1.0, b=0.0, targets=(0.0, 1.0), edges=(), ld=None, **kw):
    """[S, L] host arrays -> ops.ctr_calib's three results on the host; ``ld``: rows ``ld`` apart, NaN / label 7 between."""
    S, L = z.shape
    if ld is None:
        zd, yd = torch.from_numpy(z).cuda(), torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).cuda()
    else:
        zw = np.full((S, ld), np.nan, np.float32)
        yw = np.full((S, ld), 7, np.int32)
        zw[:, :L], yw[:, :L] = z, y
        zd, yd = torch.from_numpy(zw).cuda()[:, :L], torch.from_numpy(yw).cuda()[:, :L]
    sums, counts, bins = ops.ctr_calib(zd, yd, L, a=a, b=b, targets=targets, edges=np.asarray(edges, np.float32), **kw)
    return sums.cpu().numpy(), counts.cpu().numpy(), bins.cpu().numpy()


def _check(z, y, got, a=1.0, b=0.0, targets=(0.0, 1.0), edges=(), exact_from=None, what=""):
    sums, counts, bins = got
    rs, ra, rc, rb = calib_oracle_rows(z, y, a=a, b=b, targets=targets, edges=edges)
    assert sums.dtype == np.float64 and counts.dtype == np.int64 and bins.dtype == np.int64
    assert np.array_equal(counts, rc), (what, counts, rc)
    assert np.array_equal(bins[:, :, :2], rb[:, :, :2]), (what, np.argwhere(bins[:, :, :2] != rb[:, :, :2])[:8])
    dm = np.abs(bins[:, :, 2] - rb[:, :, 2])
    bound = sum_bound(rc[:, :1], ra)
    err = np.abs(sums - rs)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"{what}: max |sum - oracle| / bound per column = {np.round(ratio.max(axis=0), 4).tolist()}, "
          f"max mass difference / count = {np.max(dm / np.maximum(rb[:, :, 0], 1)):.3f}")
    assert (dm <= 2 * rb[:, :, 0]).all(), (what, dm.max())
    if exact_from is not None:
        assert np.array_equal(sums[:, exact_from:], rs[:, exact_from:]), (what, sums, rs)
        err, bound = err[:, :exact_from], bound[:, :exact_from]
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[:8], err.max())


@pytest.mark.parametrize("L", SEG_LENS)
def test_shapes_rows_and_bins(hip_lib, L):
    rng = np.random.default_rng(L)
    vals = np.concatenate([np.arange(-36, 37) / 8, [-0.0, 0.0, -0.0]]).astype(np.float32)     # every edge is present
    for S, n_bins in ((2, 1), (3, 2), (2, 10), (3, 64)):
        z = rng.choice(vals, (S, L))
        y = rng.integers(0, 2, (S, L))
        e = _edges(n_bins)
        _check(z, y, _run(z, y, edges=e, ld=L + 37), edges=e, what=f"L={L} S={S} n_bins={n_bins}")


def test_signed_zero_on_an_edge(hip_lib):
    z = np.array([[-0.0, 0.0, -0.0, np.float32(-1e-45), np.float32(1e-45)]], np.float32)
    y = np.array([[1, 0, 1, 0, 1]])
    for e in (np.array([0.0], np.float32), np.array([-0.0], np.float32)):
        _, _, bins = _run(z, y, edges=e)
        assert bins[0, :, 0].tolist() == [1, 4] and bins[0, :, 1].tolist() == [0, 3]


def test_exact_dyadic_sums(hip_lib):
    rng = np.random.default_rng(1)
    for S, L in ((3, 10000), (5, 257)):
        z = rng.integers(-8, 9, (S, L)).astype(np.float32)
        y = rng.integers(0, 2, (S, L))
        e = _edges(10)
        got = _run(z, y, a=0.0, b=0.0, edges=e)
        _check(z, y, got, a=0.0, b=0.0, edges=e, exact_from=1, what=f"exact S={S} L={L}")
        n = S * [L]
        assert np.abs(got[0][:, 0] - np.array(n) * np.log(2.0)).max() <= (L + 16) * 2.0 ** -53 * L * np.log(2.0)
        assert np.array_equal(got[2][:, :, 2], got[2][:, :, 0] << 39)          # p = 1/2 exactly


def _families(rng, S, L):
    mix = rng.choice(np.array([88, -88, 104, -104, 1e38, -1e38, 0.5, -2.0], np.float32), (S, L))
    return {"scale1": rng.normal(size=(S, L)).astype(np.float32),
            "scale30": (30 * rng.normal(size=(S, L))).astype(np.float32),
            "mix": mix}


@pytest.mark.parametrize("a,b", MAPS)
def test_real_valued_sums_within_the_bound(hip_lib, a, b):
    rng = np.random.default_rng(2)
    for S, L in ((1, 20011), (3, 4500)):
        y = rng.integers(0, 2, (S, L))
        for name, z in _families(rng, S, L).items():
            for targets in ((0.0, 1.0), platt_targets(y)):
                e = ops.calib_edges(10, a, b)
                _check(z, y, _run(z, y, a=a, b=b, targets=targets, edges=e), a=a, b=b, targets=targets, edges=e,
                       what=f"{name} a={a} b={b} targets={targets[0]:.4g},{targets[1]:.4g} S={S} L={L}")


def test_invalid_pairs_are_counted_and_left_out(hip_lib):
    rng = np.random.default_rng(3)
    S, L = 2, 5000
    z = rng.normal(size=(S, L)).astype(np.float32)
    y = rng.integers(0, 2, (S, L))
    z[0, 3], z[0, 4097], z[1, 70], z[1, L - 1] = np.nan, np.inf, -np.inf, np.nan
    y[0, 9], y[1, 4999], y[1, 70] = 2, -1, 2                   # pair (1, 70) is bad twice
    e = _edges(10)
    got = _run(z, y, edges=e)
    assert got[1].tolist() == [[L - 3, 3], [L - 2, 4]]
    assert got[2][:, :, 0].sum(axis=1).tolist() == [L - 3, L - 2]
    _check(z, y, got, edges=e, what="invalid pairs")
    with pytest.raises(ValueError, match="segment 0"):
        ops.ctr_calibration_from_sums(*got)


def test_same_bits_on_every_launch_and_for_every_max_groups(hip_lib):
    rng = np.random.default_rng(4)
    for S, L in ((3, 9000), (40, 300), (1, 70001)):
        z = (3 * rng.normal(size=(S, L))).astype(np.float32)
        y = rng.integers(0, 2, (S, L))
        e = _edges(64)
        ref = _run(z, y, a=0.7, b=0.1, edges=e)
        for kw in ({}, {"max_groups": 1}, {"max_groups": 3}):
            got = _run(z, y, a=0.7, b=0.1, edges=e, **kw)
            for r, g in zip(ref, got):
                assert r.tobytes() == g.tobytes(), (S, L, kw)


def test_ops_checks(hip_lib):
    z = torch.zeros(8, device="cuda")
    y = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="ascending"):
        ops.ctr_calib(z, y, 8, edges=np.array([1.0, 0.0], np.float32))
    with pytest.raises(ValueError, match="n_bins"):
        ops.ctr_calib(z, y, 8, edges=np.arange(64, dtype=np.float32))
    with pytest.raises(ValueError, match="whole segments"):
        ops.ctr_calib(z, y, 3)
    sums, counts, bins = ops.ctr_calib(z, y, 8)
    assert tuple(sums.shape) == (1, 8) and tuple(counts.shape) == (1, 2) and tuple(bins.shape) == (1, 1, 3)
    assert counts.cpu().tolist() == [[8, 0]] and bins.cpu().tolist() == [[[8, 0, 8 << 39]]]
