"""-m gpu: mvin_rank_head_offset (ops.rank_head(..., offset=)) alone against float64 evaluated on the same fp32 inputs
(tests/rank_offset_ref.py), beside tests/test_gpu_rank_head.py, whose row and validity generators and whose tolerance rule
this module takes over.

Inputs.  (G, D) in {(2, 8), (3, 12), (5, 64), (33, 128), (64, 12), (64, 128)}, which select the (L2, NP) instances (1, 1),
(2, 1), (4, 1) and (5, 8) of the kernel (tests/rank_head_shapes.py restates the rule), and EXTRA, one shape for each of the
other eight: (8, 24) for (3, 1), with lanes that hold no chunk of the row and G a power of two; (64, 24) for (3, 2); (17, 36)
for (4, 2); (33, 64) for (4, 4); (5, 128) for (5, 1); (9, 68) for (5, 2); (17, 100) for (5, 4); (5, 4) and (33, 4) for (0, 1),
where a workgroup's 408 / 448 slots take phase 2 -- the loop that loads the offsets -- through a second trip.
tests/test_rank_head_shapes_host.py holds the list to that without a GPU.  Every shape runs at n_groups in {1, 7, 1025}; validity random at 80 % with every third group's negatives all masked.  Offset contents:
  "logq"        log(n_g * q), q log-uniform in [1e-7, 0.5], n_g the group's valid negatives; slot 0 carries 0, as
                data_prep.rank_offsets writes it; on scores of O(10);
  "pm80"        +-80 on the +-80 scores, so that z = s - offset reaches +-160; slot 0 carries one too;
  "nan_masked"  the logq values with NaN / +inf / -inf written into every invalid slot.

Tolerance (derived, not fitted): the rule of tests/test_gpu_rank_head.py.  The yardstick is the same formulas in numpy float32
(rank_head_offset_ref(dtype=float32)), its error against float64 measured on this module's own inputs as a maximum per
content class; the kernel may have at most 4 x that error, with a floor of 2^-23 in the quantity's unit (dscore: |err| / scale;
du, di: |err| / (scale * largest |entry| of the rows); loss: |err| / max(1, |loss|)).
Exact properties are asserted exactly.

Measured on the MI355X (yardstick over all 15 shapes: dscore 1.6e-06 / 8.5e-06 / 1.5e-06, du/di 8.2e-07 / 5.0e-06 / 8.9e-07,
loss 8.8e-07 / 8.3e-07 / 7.9e-07 for logq / pm80 / nan_masked).  Worst kernel error / bound (bound = max(4 x yardstick, floor)):
  the EXTRA shapes   dscore 0.21   du/di 0.25   loss 0.30
  the first six      dscore 0.20   du/di 0.26   loss 0.27
"""
import numpy as np
import pytest
import torch

import rank_loss_ref as rl
import rank_offset_ref as ro
from test_gpu_rank_head import FLOOR, errors, make_rows, make_valid

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8), (3, 12), (5, 64), (33, 128), (64, 12), (64, 128)]
# one shape per (L2, NP) instance of the kernel that the six above leave out (tests/rank_head_shapes.py has the rule); the two at
# D = 4 run phase 2 -- where the offsets are loaded -- in two trips
EXTRA = [(8, 24),                             # (3, 1): 6 of 8 lanes hold a chunk; G a power of two
         (64, 24),                            # (3, 2)
         (17, 36),                            # (4, 2)
         (33, 64),                            # (4, 4)
         (5, 128),                            # (5, 1)
         (9, 68),                             # (5, 2)
         (17, 100),                           # (5, 4)
         (5, 4), (33, 4)]                     # (0, 1): 408 and 448 slots of phase 2, two trips
SHAPES += EXTRA
NGROUPS = (1, 7, 1025)
CONTENT = ("logq", "pm80", "nan_masked")
SCORES = {"logq": "o10", "pm80": "pm80", "nan_masked": "o10"}
DEV = "cuda:0"


def make_offset(G, D, content, n_groups, val):
    rng = np.random.default_rng(31 * n_groups + 1009 * G + D + 7 * CONTENT.index(content))
    mask = rl.valid_mask(val, n_groups, G)
    if content == "pm80":
        return rng.choice([-80.0, 80.0], size=n_groups * G).astype(np.float32)
    q = np.exp(rng.uniform(np.log(1e-7), np.log(0.5), size=(n_groups, G)))
    n_g = np.maximum(mask[:, 1:].sum(axis=1, keepdims=True), 1)
    off = np.log(n_g * q)
    off[:, 0] = 0.0
    off = off.astype(np.float32)
    if content == "nan_masked":
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        off[~mask] = bad[np.arange(int((~mask).sum())) % 3]
    return off.reshape(-1)


def case_inputs(G, D, content, n):
    u, v = make_rows(G, D, SCORES[content], n)
    val = make_valid(G, D, "dead_groups", n)
    return u, v, val, make_offset(G, D, content, n, val)


def yardstick_run(u, v, val, off, G, mode, scale):
    y = ro.rank_head_offset_ref((u, v), val, off, G, mode, dtype=np.float32)
    s32 = np.float32(scale)
    ds = y.dscore * s32
    return {"dscore": ds, "du": ds[:, None] * v, "di": ds[:, None] * u, "loss": np.float32(y.loss * s32)}


@pytest.fixture(scope="module")
def yardstick():
    """content -> [dscore, du/di, loss] maxima of the float32 yardstick's error over every case of this module; computed once."""
    worst = {ck: [0.0, 0.0, 0.0] for ck in CONTENT}
    for G, D in SHAPES:
        for ck in CONTENT:
            for n in NGROUPS:
                u, v, val, off = case_inputs(G, D, ck, n)
                for mode in ro.MODES:
                    ref = ro.rank_head_offset_ref((u, v), val, off, G, mode)
                    e = errors(yardstick_run(u, v, val, off, G, mode, 1.0 / n), ref, u, v, 1.0 / n)
                    worst[ck] = [max(a, b) for a, b in zip(worst[ck], e)]
    for ck in CONTENT:
        print(f"float32 yardstick, offsets {ck}: dscore {worst[ck][0]:.3e}  du/di {worst[ck][1]:.3e}  loss {worst[ck][2]:.3e}")
    return worst


def run_kernel(u, v, val, off, G, mode, scale, plain=False):
    """``off`` None with ``plain``: the call without the keyword (the mvin_rank_head symbol); None without: offset=None."""
    from mvin_amd import ops
    tu, tv = torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)
    tval = None if val is None else torch.from_numpy(val).to(DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    kw = {} if plain else {"offset": None if off is None else torch.from_numpy(off).to(DEV)}
    scores, dscore, du, di = ops.rank_head(tu, tv, G, mode, scale, loss, valid=tval, counts=cnt, **kw)
    torch.cuda.synchronize()
    return {"scores": scores.cpu().numpy(), "dscore": dscore.cpu().numpy(), "du": du.cpu().numpy(), "di": di.cpu().numpy(),
            "loss": float(loss.item()), "counts": tuple(cnt.cpu().tolist())}


def same_bits(a, b, keys=("scores", "dscore", "du", "di")):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)


@pytest.mark.parametrize("G,D", SHAPES)
def test_head_with_offsets_matches_float64(G, D, yardstick, hip_lib):
    worst = {}
    for ck in CONTENT:
        for n in NGROUPS:
            u, v, val, off = case_inputs(G, D, ck, n)
            scale = 1.0 / n
            mask = rl.valid_mask(val, n, G).reshape(-1)
            for mode in ro.MODES:
                got = run_kernel(u, v, val, off, G, mode, scale)
                ref = ro.rank_head_offset_ref((u, v), val, off, G, mode)
                where = (G, D, n, ck, mode)
                assert not got["dscore"][~mask].any() and not got["du"][~mask].any() and not got["di"][~mask].any(), where
                assert got["counts"] == rl.pair_counts(got["scores"], val, G), where             # raw scores
                assert np.array_equal(got["du"], got["dscore"][:, None] * v), where
                assert np.array_equal(got["di"], got["dscore"][:, None] * u), where
                assert all(np.isfinite(got[k]).all() for k in ("scores", "dscore", "du", "di")) and np.isfinite(got["loss"]), where
                e = errors(got, ref, u, v, scale)
                worst[ck] = [max(a, b) for a, b in zip(worst.get(ck, [0.0] * 3), e)]
                for name, err, y in zip(("dscore", "du/di", "loss"), e, yardstick[ck]):
                    assert err <= max(4.0 * y, FLOOR), f"{where}: {name} error {err:.3e}, float32 yardstick {y:.3e}"
    for ck, e in worst.items():
        print(f"G={G} D={D} offsets {ck}: kernel dscore {e[0]:.3e} du/di {e[1]:.3e} loss {e[2]:.3e}  "
              f"(yardstick {yardstick[ck][0]:.3e} {yardstick[ck][1]:.3e} {yardstick[ck][2]:.3e})")


@pytest.mark.parametrize("G,D", SHAPES)
def test_no_offset_and_zero_offset_are_the_head_of_today(G, D, hip_lib):
    for n in (7, 1025):
        u, v, val, off = case_inputs(G, D, "logq", n)
        for mode in ro.MODES:
            plain = run_kernel(u, v, val, None, G, mode, 0.125, plain=True)
            none = run_kernel(u, v, val, None, G, mode, 0.125)
            zeros = run_kernel(u, v, val, np.zeros_like(off), G, mode, 0.125)
            assert same_bits(plain, none) and same_bits(plain, zeros), (n, mode)
            assert plain["counts"] == none["counts"] == zeros["counts"]
            # with a real offset: other gradients, the same raw scores and counts
            real = run_kernel(u, v, val, off, G, mode, 0.125)
            assert same_bits(plain, real, keys=("scores",)) and real["counts"] == plain["counts"], (n, mode)
            assert not np.array_equal(real["dscore"], plain["dscore"]), (n, mode)


@pytest.mark.parametrize("G,D", SHAPES)
def test_offsets_of_masked_slots_reach_nothing(G, D, hip_lib):
    for n in (7, 1025):
        u, v, val, off = case_inputs(G, D, "nan_masked", n)
        mask = rl.valid_mask(val, n, G).reshape(-1)
        assert not np.isfinite(off[~mask]).any() and np.isfinite(off[mask]).all() and (~mask).any()
        clean = np.where(mask, off, np.float32(0)).astype(np.float32)
        for mode in ro.MODES:
            a = run_kernel(u, v, val, off, G, mode, 0.125)
            b = run_kernel(u, v, val, clean, G, mode, 0.125)
            assert same_bits(a, b) and a["counts"] == b["counts"], (n, mode)
            assert all(np.isfinite(a[k]).all() for k in ("scores", "dscore", "du", "di")) and np.isfinite(a["loss"])
            assert abs(a["loss"] - b["loss"]) <= 1e-5 * max(1.0, abs(b["loss"]))                 # float atomics: order only
            assert not a["dscore"][~mask].any() and not a["du"][~mask].any() and not a["di"][~mask].any()


@pytest.mark.parametrize("G,D", SHAPES)
def test_group_bits_do_not_depend_on_the_launch(G, D, hip_lib):
    u, v, val, off = case_inputs(G, D, "logq", 1025)
    for mode in ro.MODES:
        a = run_kernel(u, v, val, off, G, mode, 0.125)
        b = run_kernel(u, v, val, off, G, mode, 0.125)
        assert same_bits(a, b) and a["counts"] == b["counts"], mode                              # two runs: identical bits
        for g in (0, 1, 6, 500, 1023, 1024):                                                     # alone = inside the launch
            rows = slice(g * G, (g + 1) * G)
            one = run_kernel(u[rows], v[rows], val[rows], off[rows], G, mode, 0.125)
            assert all(np.array_equal(one[k].view(np.uint32), a[k][rows].view(np.uint32))
                       for k in ("scores", "dscore", "du", "di")), (mode, g)
        sub = run_kernel(u[:7 * G], v[:7 * G], val[:7 * G], off[:7 * G], G, mode, 0.125)         # another grid, same bits
        assert all(np.array_equal(sub[k].view(np.uint32), a[k][:7 * G].view(np.uint32))
                   for k in ("scores", "dscore", "du", "di")), mode


def test_ops_wrapper_refuses_a_wrong_offset(hip_lib):
    from mvin_amd import ops
    u, v, val, off = case_inputs(3, 12, "logq", 7)
    tu, tv, toff = (torch.from_numpy(x).to(DEV) for x in (u, v, off))
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="offset"):
        ops.rank_head(tu, tv, 3, "softmax", 1.0, loss, offset=toff[:-1])
    with pytest.raises(ValueError, match="offset"):
        ops.rank_head(tu, tv, 3, "softmax", 1.0, loss, offset=toff.double())
    with pytest.raises(ValueError, match="offset"):
        ops.rank_head(tu, tv, 3, "softmax", 1.0, loss, offset=torch.stack([toff, toff], dim=1)[:, 0])     # not contiguous
    with pytest.raises(ValueError, match="offset"):
        ops.rank_head(tu, tv, 3, "softmax", 1.0, loss, offset=toff.cpu())
    assert float(loss.item()) == 0.0                                    # nothing was launched
    out = ops.rank_head(tu[:0], tv[:0], 3, "softmax", 1.0, loss, offset=toff[:0])
    assert out[0].numel() == 0 and float(loss.item()) == 0.0
