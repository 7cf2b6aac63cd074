"""CPU: the host side of the training-step guard -- the oracle by hand, the step-size table, the work-table builder, argument
validation of the two entry points before anything touches a GPU, and the argument checks of Trainer / harness.train."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import grad_guard_oracle as go


# --------------------------------------------------------------------------- the oracle by hand
def test_oracle_three_four_five():
    tab = go.lr_table(0.01)
    st = go.guard(go.new_state(clip=5.0), [np.zeros(2, np.float32)], [0.0], np.array([3, 4], np.float32), tab)
    assert st["last_sumsq"] == 25.0 and st["seg_sumsq"][0] == 25.0 and st["last_norm"] == 5.0
    assert st["clipped"] == 0 and st["scale"] == np.float32(1.0) and st["ok"] == 1 and st["applied"] == 1
    assert st["lr_t"] == tab[0]
    st = go.guard(go.new_state(clip=4.999), [np.zeros(2, np.float32)], [0.0], np.array([3, 4], np.float32), tab)
    assert st["clipped"] == 1 and st["clipped_steps"] == 1
    assert st["scale"] == np.float32(float(np.float32(4.999)) / 5.0)


def test_oracle_l2_term_enters_the_element():
    x, g = np.array([2, -1], np.float32), np.array([2, 4.5], np.float32)
    e = go.elements([x], [0.5], g)[0]
    np.testing.assert_array_equal(e, np.array([3, 4], np.float32))
    # one rounding: (1 + 2^-23)^2 - (1 + 2^-22) is 2^-46 exactly; rounding the product first gives 0
    a = np.float32(1 + 2.0 ** -23)
    assert go.fmaf32(a, a, np.float32(-(1 + 2.0 ** -22))) == np.float32(2.0 ** -46)
    assert np.float32(a * a) + np.float32(-(1 + 2.0 ** -22)) == np.float32(0.0)
    # ... and a sum just above the midpoint of 1 and 1 + 2^-23 rounds up, a product below half an ulp vanishes
    assert go.fmaf32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1.0)) == np.float32(1.0)
    assert go.fmaf32(np.float32(2.0 ** -12 + 2.0 ** -30), np.float32(2.0 ** -12), np.float32(1.0)) == np.float32(1 + 2.0 ** -23)


@pytest.mark.parametrize("skip", [False, True])
def test_oracle_counts_a_nan_once(skip):
    tab = go.lr_table(0.01)
    st = go.new_state(clip=1.0, skip=skip)
    go.guard(st, [np.zeros(3, np.float32)], [0.0], np.array([1, np.nan, 2], np.float32), tab)
    assert st["last_nonfinite"] == 1 and st["clipped"] == 0 and st["scale"] == np.float32(1.0)
    assert st["ok"] == (0 if skip else 1)
    assert st["applied"] == (0 if skip else 1) and st["skipped_steps"] == (1 if skip else 0)
    assert st["finite_steps"] == 0 and st["norm_sum"] == 0.0 and math.isnan(st["last_norm"])
    if skip:
        assert st["lr_t"] == np.float32(0.0)                    # untouched
    # an infinity through the L2 term: x is inf, g finite
    st = go.guard(go.new_state(skip=skip), [np.array([np.inf, 1], np.float32)], [0.25], np.zeros(2, np.float32), tab)
    assert st["last_nonfinite"] == 1


def test_guarded_adam_skips_without_a_trace():
    p = {"a": np.array([1.0, -2.0])}
    opt = go.GuardedAdam(p, 0.1)
    q = opt.step(dict(p), {"a": np.array([0.5, 0.25], np.float32)}, scale=1.0, ok=False)
    assert opt.t == 0 and not opt.m["a"].any() and q["a"] is p["a"]
    ref = go.train_ref.AdamRef(p, 0.1, dtype=np.float64)
    a = opt.step(dict(p), {"a": np.array([0.5, 0.25], np.float32)}, scale=0.5)
    b = ref.step(dict(p), {"a": np.array([0.25, 0.125], np.float64)})
    np.testing.assert_array_equal(a["a"], b["a"])


# --------------------------------------------------------------------------- lr_table
def _trainer_like(lr=0.02, b1=0.9, b2=0.999):
    return types.SimpleNamespace(lr=lr, b1=b1, b2=b2, lr_t=None)


def test_lr_table_is_lr_t_entry_by_entry():
    from mvin_amd.training import Trainer
    tr = _trainer_like()
    tr.lr_t = lambda t: Trainer.lr_t(tr, t)
    tab = Trainer.lr_table(tr)
    assert tab.dtype == np.float32
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    T = len(tab)
    assert b1 ** T < 2.0 ** -54 and b2 ** T < 2.0 ** -54
    assert b1 ** (T - 1) >= 2.0 ** -54 or b2 ** (T - 1) >= 2.0 ** -54
    assert T == go.lr_table_len(0.9, 0.999) and 37000 < T < 38000
    for t in range(1, T + 1):
        assert tab[t - 1] == np.float32(Trainer.lr_t(tr, t)), t
    assert tab[-1] == np.float32(tr.lr) and Trainer.lr_t(tr, T) == tr.lr
    np.testing.assert_array_equal(tab, go.lr_table(0.02))
    # a short table: beta2 decides
    tr2 = _trainer_like(lr=0.5, b1=0.5, b2=0.25)
    tr2.lr_t = lambda t: Trainer.lr_t(tr2, t)
    assert len(Trainer.lr_table(tr2)) == 55 == go.lr_table_len(0.5, 0.25)


def test_lr_table_refuses_a_beta_it_cannot_tabulate():
    from mvin_amd.training import Trainer
    tr = _trainer_like(b2=1 - 1e-9)
    tr.lr_t = lambda t: Trainer.lr_t(tr, t)
    with pytest.raises(ValueError):
        Trainer.lr_table(tr)
    tr = _trainer_like(b2=1 - 1e-6)           # a float32 below 1, but 3.7e7 entries
    tr.lr_t = lambda t: Trainer.lr_t(tr, t)
    with pytest.raises(ValueError, match="2\\*\\*20"):
        Trainer.lr_table(tr)


# --------------------------------------------------------------------------- work table
@pytest.mark.parametrize("nseg", [1, 7, 256])
def test_work_items_tile_the_flat_range(nseg):
    from mvin_amd import ops
    segments = go.segments_of(go.guard_lengths(nseg))
    items = ops.guard_work_items(segments)
    assert items.dtype.itemsize == 16
    assert go.work_items_ok(items, segments) is None
    total = sum(n for _, n in segments)
    assert int(items["len"].sum()) == total and len(items) <= total / 4096 + nseg
    assert items["len"].max() <= 4096


def test_work_items_of_awkward_tables():
    from mvin_amd import ops
    for segments in ([(0, 4096)], [(0, 4097)], [(0, 1), (1, 0), (1, 8192), (8193, 2)], [(0, 5), (5, 4096 * 2 + 1)]):
        assert go.work_items_ok(ops.guard_work_items(segments), segments) is None
    assert go.work_items_ok(ops.guard_work_items([(0, 8192)])[:1], [(0, 8192)]) is not None          # the checker checks


# --------------------------------------------------------------------------- ABI
def test_entry_points_validate_before_launching(hip_lib):
    one = C.c_void_p(16)
    g = lambda **kw: hip_lib.mvin_grad_guard(*[kw.get(k, d) for k, d in (
        ("segs", one), ("nseg", 3), ("total", 100), ("g", one), ("items", one), ("nitems", 3), ("partials", one),
        ("lr", one), ("T", 10), ("state", one), ("cap", 0), ("stream", None))])
    for k in ("segs", "g", "items", "partials", "lr", "state"):
        assert g(**{k: None}) == -1, k
        assert b"null" in hip_lib.mvin_last_error()
    assert g(nseg=257) == -2 and b"nseg=257" in hip_lib.mvin_last_error()
    assert g(nseg=0) == -2
    assert g(nitems=0) == -2 and b"empty work table" in hip_lib.mvin_last_error()
    assert g(T=0) == -2 and g(total=0) == -2 and g(cap=-1) == -2
    a = lambda **kw: hip_lib.mvin_l2_adam_multi_guarded(*[kw.get(k, d) for k, d in (
        ("segs", one), ("nseg", 3), ("total", 100), ("g", one), ("m", one), ("v", one), ("loss", one), ("apply", 1),
        ("state", one), ("b1", 0.9), ("b2", 0.999), ("eps", 1e-8), ("stream", None))])
    for k in ("segs", "g", "state", "m", "v"):
        assert a(**{k: None}) == -1, k
    assert a(nseg=257) == -2 and b"nseg=257" in hip_lib.mvin_last_error()
    assert a(total=0) == -2


def test_state_block_layout_matches_the_header():
    from mvin_amd import ops
    f = ops.GUARD_STATE.fields
    assert ops.GUARD_STATE.itemsize == 104 + 8 * 256 and f["seg_sumsq"][1] == 104
    assert [f[k][1] for k in ("clip", "skip", "ok", "clipped", "scale", "lr_t", "steps", "applied", "norm_sum")] == \
        [0, 4, 8, 12, 16, 20, 24, 48, 72]
    assert ops.GUARD_ITEM.itemsize == ops.GUARD_PARTIAL.itemsize == 16


# --------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("bad", [0, -1, float("nan"), float("inf"), 0.0, "1", True])
def test_clip_norm_is_checked(bad):
    from mvin_amd import harness
    from mvin_amd.training import Trainer, check_clip_norm
    with pytest.raises(ValueError, match="clip_norm"):
        check_clip_norm(bad)
    with pytest.raises(ValueError, match="clip_norm"):
        Trainer(None, clip_norm=bad)
    with pytest.raises(ValueError, match="clip_norm"):
        harness.train(None, None, clip_norm=bad)


def test_good_guard_arguments_pass_the_check():
    from mvin_amd import harness
    from mvin_amd.training import check_clip_norm
    assert check_clip_norm(None) is None and check_clip_norm(5) == 5.0 and check_clip_norm(np.float32(0.5)) == 0.5
    with pytest.raises(ValueError, match="skip_nonfinite"):
        harness.train(None, None, skip_nonfinite="yes")
