"""-m gpu: mvin_rank_head (ops.rank_head) alone against float64 evaluated on the same fp32 inputs (tests/rank_loss_ref.py).

Inputs.  G in {2, 3, 5, 33, 64} x D in {8, 12, 64, 128}, and the shapes of EXTRA, x n_groups in {1, 7, 1025} (groups straddle
waves and workgroups).  The kernel is compiled once per (L2, NP) -- 2^L2 lanes per row, NP passes over a group's rows
(tests/rank_head_shapes.py restates the rule) -- and the product reaches six of the twelve instances; EXTRA holds the smallest
shapes for the rest and for three paths the product never takes:
  (3, 1)  (3, 20), (8, 24), (32, 32)    (3, 2)  (33, 32), (64, 24)    (4, 2)  (17, 36), (32, 64)
  (5, 2)  (9, 68), (16, 128)            (5, 4)  (17, 100), (32, 128)  -- at D = 20, 24, 36, 68 and 100 lanes of a row's
          lane group hold no chunk (D / 4 is no power of two), at D = 32, 64 and 128 every lane does;
  (0, 1)  (3, 4), (5, 4), (33, 4), (64, 4): D = 4, where a workgroup holds more slots than lanes (340, 408, 448) and phase 2
          takes a second trip, dscore overwriting the scores in LDS between the two; (64, 4) is exactly 256 slots, one trip;
  (4, 8), (16, 64): G a power of two in 4..32 (with 8 and 32 above) at (1, 1) and (4, 1) -- the segment of phase 2 is exactly
          G lanes wide, no slot lane is idle.
tests/test_rank_head_shapes_host.py holds the list to all that without a GPU.  Validity absent / random at 80 % / random plus
every third group with all its negatives masked; rows scaled so that the scores are O(1), O(10) or +-80; a quarter of the groups have rows of small
dyadic entries, whose dot products are exact in any order, so exact ties occur.  Every (validity, score content) pair runs for
every (G, D) under both objectives; every (G, D) runs at all three launch sizes (``plan``: which pair takes the 1025-group
launch rotates with the shape).

Tolerance (derived, not fitted).  The yardstick is the same formulas evaluated straightforwardly in numpy float32
(rank_head_ref(dtype=float32): row dot product, max-subtracted softmax, stable softplus, the group losses added up in group
order).  Its error against float64 is measured on this module's own inputs, as a maximum per score-content class (a maximum
over many elements is a stable statistic; the error of one small case is not).  The kernel may have at most 4 x that error
-- the factor covers another summation order and another exp / log -- with a floor of 2^-23 in the quantity's unit:
  dscore   |err| / scale;              du, di   |err| / (scale * largest |entry| of the case's rows);
  loss     |err| / max(1, |loss|).
Exact properties are asserted exactly: masked dscore / du / di are 0, the counts equal the integers computed on the host from
the kernel's OWN scores, du / di are the single fp32 products of the kernel's own dscore with the rows, a group evaluated alone
has the bits it has inside the 1025-group launch, and two runs agree bit for bit.

Measured on the MI355X (yardstick over all 37 shapes: dscore 2.2e-07 / 1.4e-06 / 5.9e-06, du/di 1.2e-07 / 8.6e-07 / 3.4e-06,
loss 7.5e-07 / 9.7e-07 / 4.7e-06 for o1 / o10 / pm80).  Worst kernel error / bound (bound = max(4 x yardstick, floor)):
  the EXTRA shapes   dscore 0.19   du/di 0.24   loss 0.29
  the product        dscore 0.22   du/di 0.26   loss 0.24
The kernel is about as accurate as the float32 restatement at every instance; no shape came near its bound.
"""
import functools

import numpy as np
import pytest
import torch

import rank_loss_ref as rl

pytestmark = pytest.mark.gpu

GS = (2, 3, 5, 33, 64)
DS = (8, 12, 64, 128)
# shapes beside the product GS x DS: the smallest that reach what the product misses (tests/rank_head_shapes.py has the rule,
# tests/test_rank_head_shapes_host.py holds this list to it)
EXTRA = [(3, 20), (8, 24), (32, 32),          # (3, 1): idle lanes (5, 6 of 8 chunks) and full lanes; G a power of two
         (33, 32), (64, 24),                  # (3, 2)
         (17, 36), (32, 64),                  # (4, 2)
         (9, 68), (16, 128),                  # (5, 2)
         (17, 100), (32, 128),                # (5, 4)
         (3, 4), (5, 4), (33, 4), (64, 4),    # (0, 1); phase 2 in two trips (340, 408, 448 slots), and exactly one (256)
         (4, 8), (16, 64)]                    # G a power of two at (1, 1) and (4, 1)
SHAPES = [(G, D) for G in GS for D in DS] + EXTRA
NGROUPS = (1, 7, 1025)
VALIDITY = ("absent", "random80", "dead_groups")
CONTENT = ("o1", "o10", "pm80")
FLOOR = 2.0 ** -23


@functools.lru_cache(maxsize=9)
def make_rows(G, D, content, n_groups):
    """(u, v) float32 [n_groups * G, D].  Scores: o1 / o10 -- u.v of normal rows scaled to a standard deviation of 1 / 10;
    pm80 -- v = +-80 u / |u|^2 plus a perturbation, so u.v = +-80 + O(1).  Every fourth group: small dyadic entries."""
    rng = np.random.default_rng(100000 * n_groups + 1000 * G + D + {"o1": 0, "o10": 1, "pm80": 2}[content] * 7919)
    B = n_groups * G
    u = rng.normal(size=(B, D))
    v = rng.normal(size=(B, D))
    if content == "pm80":
        sign = rng.choice([-80.0, 80.0], size=(B, 1))
        v = sign * u / (u * u).sum(axis=1, keepdims=True) + 0.3 * v / np.sqrt(D)
    else:
        v *= {"o1": 1.0, "o10": 10.0}[content] / np.sqrt(D)
    quant = np.repeat(np.arange(n_groups) % 4 == 3, G)
    amp = {"o1": 0.5, "o10": 2.0, "pm80": 4.0}[content]
    u[quant] = rng.integers(-2, 3, size=(int(quant.sum()), D)) * 0.5
    v[quant] = rng.integers(-2, 3, size=(int(quant.sum()), D)) * (amp / 2.0)
    return np.ascontiguousarray(u, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)


@functools.lru_cache(maxsize=9)
def make_valid(G, D, kind, n_groups):
    if kind == "absent":
        return None
    rng = np.random.default_rng(100000 * n_groups + 77 * G + D)
    val = (rng.random((n_groups, G)) < 0.8).astype(np.float32)
    if kind == "dead_groups":
        val[::3, 1:] = 0.0
    val[:, 0] = 1.0
    return val.reshape(-1)


def plan(G, D):
    """The (validity, content, n_groups) triples of one (G, D): all nine pairs; ONE of them at 1025 groups -- which one rotates
    with (G, D), so every pair meets the large launch under several shapes -- the others at 1 and 7 groups in turn."""
    big = SHAPES.index((G, D)) % 9
    pairs = [(vk, ck) for vk in VALIDITY for ck in CONTENT]
    return [(vk, ck, 1025 if k == big else (1, 7)[(k + big) % 2]) for k, (vk, ck) in enumerate(pairs)]


def case_inputs(G, D, vk, ck, n):
    return make_rows(G, D, ck, n) + (make_valid(G, D, vk, n),)


def errors(got, ref64, u, v, scale):
    """(dscore, du/di, loss) errors of ``got`` (fp32 results for scale ``scale``) in the units of the module docstring."""
    rowmax = max(float(np.abs(u).max()), float(np.abs(v).max()))
    e_ds = float(np.abs(got["dscore"].astype(np.float64) - ref64.dscore * scale).max()) / scale
    e_du = max(float(np.abs(got["du"].astype(np.float64) - ref64.du * scale).max()),
               float(np.abs(got["di"].astype(np.float64) - ref64.di * scale).max())) / (scale * rowmax)
    L = float(ref64.loss) * scale
    e_loss = abs(float(got["loss"]) - L) / max(1.0, abs(L))
    return e_ds, e_du, e_loss


def yardstick_run(u, v, val, G, mode, scale):
    y = rl.rank_head_ref((u, v), val, G, mode, dtype=np.float32)
    s32 = np.float32(scale)
    ds = y.dscore * s32
    return {"dscore": ds, "du": ds[:, None] * v, "di": ds[:, None] * u, "loss": np.float32(y.loss * s32)}


@pytest.fixture(scope="module")
def yardstick():
    """content -> [dscore, du/di, loss] maxima of the float32 yardstick's error over every case of this module; computed once."""
    worst = {ck: [0.0, 0.0, 0.0] for ck in CONTENT}
    for G, D in SHAPES:
        for vk, ck, n in plan(G, D):
            u, v, val = case_inputs(G, D, vk, ck, n)
            for mode in rl.MODES:
                ref = rl.rank_head_ref((u, v), val, G, mode)
                e = errors(yardstick_run(u, v, val, G, mode, 1.0 / n), ref, u, v, 1.0 / n)
                worst[ck] = [max(a, b) for a, b in zip(worst[ck], e)]
    for ck in CONTENT:
        print(f"float32 yardstick, scores {ck}: dscore {worst[ck][0]:.3e}  du/di {worst[ck][1]:.3e}  loss {worst[ck][2]:.3e}")
    return worst


def run_kernel(u, v, val, G, mode, scale, counts=True):
    from mvin_amd import ops
    dev = "cuda:0"
    tu, tv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    tval = None if val is None else torch.from_numpy(val).to(dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev) if counts else None
    scores, dscore, du, di = ops.rank_head(tu, tv, G, mode, scale, loss, valid=tval, counts=cnt)
    torch.cuda.synchronize()
    return {"scores": scores.cpu().numpy(), "dscore": dscore.cpu().numpy(), "du": du.cpu().numpy(), "di": di.cpu().numpy(),
            "loss": float(loss.item()), "counts": None if cnt is None else tuple(cnt.cpu().tolist())}


@pytest.mark.parametrize("G,D", SHAPES)
def test_head_matches_float64(G, D, yardstick, hip_lib):
    worst = {}
    for vk, ck, n in plan(G, D):
        u, v, val = case_inputs(G, D, vk, ck, n)
        scale = 1.0 / n
        mask = rl.valid_mask(val, n, G).reshape(-1)
        for mode in rl.MODES:
            got = run_kernel(u, v, val, G, mode, scale)
            ref = rl.rank_head_ref((u, v), val, G, mode)
            where = (G, D, n, vk, ck, mode)
            # exact properties
            assert not got["dscore"][~mask].any() and not got["du"][~mask].any() and not got["di"][~mask].any(), where
            assert got["counts"] == rl.pair_counts(got["scores"], val, G), where
            assert np.array_equal(got["du"], got["dscore"][:, None] * v) and np.array_equal(got["di"], got["dscore"][:, None] * u), where
            assert np.isfinite(got["dscore"]).all() and np.isfinite(got["loss"]), where
            # scores: a D-term fp32 dot product, |err| <= D 2^-24 sum |u_k v_k|
            bound = D * 2.0 ** -24 * (np.abs(u.astype(np.float64)) * np.abs(v.astype(np.float64))).sum(axis=1)
            assert (np.abs(got["scores"] - ref.scores) <= bound + 1e-30).all(), where
            e = errors(got, ref, u, v, scale)
            worst[ck] = [max(a, b) for a, b in zip(worst.get(ck, [0.0] * 3), e)]
            for name, err, y in zip(("dscore", "du/di", "loss"), e, yardstick[ck]):
                assert err <= max(4.0 * y, FLOOR), f"{where}: {name} error {err:.3e}, float32 yardstick {y:.3e}"
    for ck, e in worst.items():
        print(f"G={G} D={D} scores {ck}: kernel dscore {e[0]:.3e} du/di {e[1]:.3e} loss {e[2]:.3e}  "
              f"(yardstick {yardstick[ck][0]:.3e} {yardstick[ck][1]:.3e} {yardstick[ck][2]:.3e})")


def test_ties_occur_and_are_counted(hip_lib):
    """The dyadic groups produce exact ties between a negative and its positive, and the kernel counts them as one."""
    u, v, _ = case_inputs(5, 8, "absent", "o1", 1025)
    got = run_kernel(u, v, None, 5, "bpr", 1.0)
    s = got["scores"].reshape(-1, 5)
    ties = int(np.count_nonzero(s[:, 1:] == s[:, :1]))
    assert ties > 20
    below = int(np.count_nonzero(s[:, 1:] < s[:, :1]))
    assert got["counts"] == (2 * below + ties, 1025 * 4)
    assert run_kernel(u, v, None, 5, "bpr", 1.0, counts=False)["counts"] is None       # the counts are optional


@pytest.mark.parametrize("G,D", [(2, 8), (3, 12), (5, 64), (33, 128), (64, 12), (64, 128)] + EXTRA)
def test_group_bits_do_not_depend_on_the_launch(G, D, hip_lib):
    u, v, val = case_inputs(G, D, "dead_groups", "o10", 1025)
    for mode in rl.MODES:
        a = run_kernel(u, v, val, G, mode, 0.125)
        b = run_kernel(u, v, val, G, mode, 0.125)
        for k in ("scores", "dscore", "du", "di"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (mode, k)       # two runs: identical bits
        assert a["counts"] == b["counts"]
        for g in (0, 1, 6, 500, 1023, 1024):                                                   # alone = inside the launch
            rows = slice(g * G, (g + 1) * G)
            one = run_kernel(u[rows], v[rows], val[rows], G, mode, 0.125)
            for k in ("scores", "dscore", "du", "di"):
                assert np.array_equal(one[k].view(np.uint32), a[k][rows].view(np.uint32)), (mode, k, g)
        sub = run_kernel(u[:7 * G], v[:7 * G], val[:7 * G], G, mode, 0.125)                     # another grid, same bits
        for k in ("scores", "dscore", "du", "di"):
            assert np.array_equal(sub[k].view(np.uint32), a[k][:7 * G].view(np.uint32)), (mode, k)


def test_loss_accumulates_and_empty_batch_is_a_no_op(hip_lib):
    from mvin_amd import ops
    u, v, val = case_inputs(3, 8, "random80", "o1", 7)
    dev = "cuda:0"
    tu, tv, tval = (torch.from_numpy(x).to(dev) for x in (u, v, val))
    loss = torch.full((1,), 2.5, dtype=torch.float32, device=dev)
    cnt = torch.tensor([10, 20], dtype=torch.int64, device=dev)
    ops.rank_head(tu, tv, 3, "softmax", 0.5, loss, valid=tval, counts=cnt)
    ref = rl.rank_head_ref((u, v), val, 3, "softmax")
    assert abs(float(loss.item()) - (2.5 + 0.5 * float(ref.loss))) <= 1e-5
    c0, c1 = rl.pair_counts(ref.scores.astype(np.float32), val, 3)
    assert cnt[1].item() == 20 + c1
    out = ops.rank_head(tu[:0], tv[:0], 3, "softmax", 0.5, loss, counts=cnt)
    assert out[0].numel() == 0 and cnt[1].item() == 20 + c1
    with pytest.raises(ValueError, match="whole groups"):
        ops.rank_head(tu[:4], tv[:4], 3, "softmax", 0.5, loss)
