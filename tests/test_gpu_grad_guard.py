"""-m gpu: the two kernels of the training-step guard on their own (mvin_grad_guard, mvin_l2_adam_multi_guarded through
their mvin_amd.ops wrappers) against tests/grad_guard_oracle.py.

Shapes: 1, 7 and 256 segments whose lengths mix multiples of 4 with 1, 3, 5, 4095, 4096, 4097 and 3 * 4096 + 5 (work items of
at most 4096 elements: full items, ragged tails, several items per segment), some segments stored off a 16-byte boundary in
a padded buffer, L2 coefficients cycling through (0.5, 0, 2, 0.25).

Bounds.
  * EXACT cases: integer g in [-4, 4] and integer x in [-3, 3], so every e = g + l2 x is a multiple of 1/4 below 16 and every
    e^2 a multiple of 1/16 below 256: all sums stay below 2^53 / 16 and are exact in double in any order -> array_equal,
    the double square root and division of the decision included (both correctly rounded, as the oracle's).
  * real-valued sumsq: |got - fsum| <= n * 2^-53 * fsum, the worst case of any-order double summation of n non-negative
    terms (the squares themselves are exact).  Derived, not measured.
  * scale: 2^-23 relative to the float64 oracle: one double square root, one double division, one rounding to float32.
  * guarded Adam against float64: the project's tolerance for kernels with sqrtf / division inside, 2e-4 * max|ref| + 1e-7
    per tensor, with the side condition that the same formula in float32 on the CPU stays within a quarter of it.
"""
import math

import numpy as np
import pytest
import torch

import grad_guard_oracle as go

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B1, B2, EPS = (float(np.float32(h)) for h in (0.9, 0.999, 1e-8))
LR = 0.01
_TAB = {}


def lr_tab():
    """The step-size table, host and device, computed once for the module."""
    if not _TAB:
        _TAB["host"] = go.lr_table(LR)
        _TAB["dev"] = torch.from_numpy(_TAB["host"]).to(DEV)
    return _TAB["host"], _TAB["dev"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def ints(rng, n, lo, hi):
    return rng.integers(lo, hi + 1, n).astype(np.float32)


def reals(rng, n):
    a = rng.standard_normal(n)
    return np.where(np.abs(a) < 2.0 ** -10, np.copysign(2.0 ** -10, a), a).astype(np.float32)


class Case(object):
    """Segments in one padded device buffer (gaps pre-filled with 77), their table, the work table and a partials buffer."""

    def __init__(self, lengths, real, seed):
        from mvin_amd import ops
        rng = np.random.default_rng(seed)
        self.rng, self.lengths, self.nseg = rng, list(lengths), len(lengths)
        self.l2s = [go.L2_CYCLE[i % 4] for i in range(self.nseg)]
        self.offs, pos = [], 0
        for i, n in enumerate(self.lengths):
            pos = (pos + 3) // 4 * 4 + go.MISALIGN[i % len(go.MISALIGN)]
            self.offs.append(pos)
            pos += n
        self.xs = [reals(rng, n) if real else ints(rng, n, -3, 3) for n in self.lengths]
        self.hbuf = np.full(pos + 4, 77.0, np.float32)
        self.total = int(sum(self.lengths))
        self.edges = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.items_h = ops.guard_work_items(go.segments_of(self.lengths))
        assert go.work_items_ok(self.items_h, go.segments_of(self.lengths)) is None
        self.nitems = len(self.items_h)
        self.items = dev(self.items_h.view(np.uint8))
        self.upload()

    def upload(self):
        """(Re)write the parameters into the device buffer and rebuild the segment table on it."""
        for x, o in zip(self.xs, self.offs):
            self.hbuf[o:o + x.size] = x
        self.buf = dev(self.hbuf)
        table = np.zeros(self.nseg, dtype=[("x", "<u8"), ("off", "<i8"), ("n", "<i8"), ("l2", "<f4"), ("pad", "<i4")])
        for i in range(self.nseg):
            table[i] = (self.buf.data_ptr() + 4 * self.offs[i], self.edges[i], self.lengths[i], self.l2s[i], 0)
        self.segs = dev(table.view(np.uint8))

    def params(self):
        h = host(self.buf)
        return [h[o:o + n].copy() for o, n in zip(self.offs, self.lengths)]

    def guard(self, g, state, grid_cap=0):
        """One mvin_grad_guard on the device state tensor ``state``; returns (state record, partials records)."""
        from mvin_amd import ops
        partials = torch.full((self.nitems * ops.GUARD_PARTIAL.itemsize,), 0xAB, dtype=torch.uint8, device=DEV)
        ops.grad_guard(self.segs, self.nseg, self.total, g, self.items, self.nitems, partials, lr_tab()[1], state,
                       grid_cap=grid_cap)
        return host(state).view(ops.GUARD_STATE)[0].copy(), host(partials).view(ops.GUARD_PARTIAL).copy()


def state_tensor(**fields):
    """A zeroed mvin_guard_state with ``fields`` set, on the device (uint8)."""
    from mvin_amd import ops
    st = np.zeros(1, ops.GUARD_STATE)
    st["clip"] = np.inf
    for k, v in fields.items():
        st[k] = v
    return dev(st.view(np.uint8))


def assert_state_equals(got, ref, nseg, what):
    for k in ("clip", "skip", "ok", "clipped", "scale", "lr_t", "steps", "clipped_steps", "skipped_steps", "applied",
              "last_nonfinite", "finite_steps", "norm_sum", "norm_max", "last_norm", "last_sumsq"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(got["seg_sumsq"], ref["seg_sumsq"], err_msg=f"{what}: seg_sumsq")
    assert not got["seg_sumsq"][nseg:].any()


# =============================================================================================== 1. exact
@pytest.mark.parametrize("nseg", [1, 7, 256])
def test_exact_sums_decision_and_counters_over_two_calls(nseg, hip_lib):
    c = Case(go.guard_lengths(nseg), False, 100 + nseg)
    tab = lr_tab()[0]
    state = state_tensor(clip=10.0, skip=1)
    ref = go.new_state(clip=10.0, skip=True)
    for call in range(2):
        g0 = ints(c.rng, c.total, -4, 4) * np.float32(1 + call)        # the second call's norm is the larger one
        got, partials = c.guard(dev(g0), state)
        go.guard(ref, c.xs, c.l2s, g0, tab)
        print(f"nseg={nseg} call {call}: sumsq {got['last_sumsq']!r} vs {ref['last_sumsq']!r}, scale {got['scale']!r} vs "
              f"{ref['scale']!r}, norm {got['last_norm']!r} vs {ref['last_norm']!r}")
        assert ref["last_sumsq"] * 16 == round(ref["last_sumsq"] * 16) < 2.0 ** 53, "case bug: not exact in double"
        assert_state_equals(got, ref, nseg, f"nseg={nseg} call {call}")
        assert got["last_nonfinite"] == 0 and got["clipped"] == 1 and got["ok"] == 1
        # the partials are the exact sums of their items
        es = np.concatenate(go.elements(c.xs, c.l2s, g0)).astype(np.float64)
        want = np.array([(es[f:f + n] ** 2).sum() for f, n in zip(c.items_h["first"], c.items_h["len"])])
        np.testing.assert_array_equal(partials["sumsq"], want)
        assert not partials["nonfinite"].any() and not partials["pad"].any()
    assert got["steps"] == got["applied"] == got["clipped_steps"] == got["finite_steps"] == 2 and got["skipped_steps"] == 0
    assert got["lr_t"] == tab[1]


def test_a_norm_equal_to_the_clip_is_not_clipped(hip_lib):
    """sumsq = 25 from a 3 in the first and a 4 in the last flat element (different segments, different workgroups):
    clip = 5 compares 25 > 25 exactly -- not clipped, scale 1.0f bit for bit; the float32 just below 5 clips."""
    c = Case(go.guard_lengths(7), False, 7)
    c.xs = [np.zeros(n, np.float32) for n in c.lengths]
    c.upload()
    g0 = np.zeros(c.total, np.float32)
    g0[0], g0[-1] = 3.0, 4.0
    tab = lr_tab()[0]
    for clip, clipped in ((np.float32(5.0), 0), (np.nextafter(np.float32(5.0), np.float32(0.0)), 1)):
        state, ref = state_tensor(clip=clip), go.new_state(clip=clip)
        got, _ = c.guard(dev(g0), state)
        go.guard(ref, c.xs, c.l2s, g0, tab)
        assert got["last_sumsq"] == 25.0 and got["last_norm"] == 5.0 and got["clipped"] == clipped
        assert_state_equals(got, ref, 7, f"clip={clip!r}")
        if not clipped:
            assert got["scale"].tobytes() == np.float32(1.0).tobytes()
        else:
            assert got["scale"] == np.float32(float(clip) / 5.0) < np.float32(1.0)


# =============================================================================================== 2. / 3. real-valued
def real_case():
    rng = np.random.default_rng(2024)
    lengths = go.guard_lengths(7) + [int(v) for v in rng.integers(1, 1540, 33)]
    c = Case(lengths, True, 2025)
    assert c.nseg == 40 and 40000 <= c.total <= 60000
    return c, reals(c.rng, c.total)


def test_real_valued_sums_and_scale(hip_lib):
    c, g0 = real_case()
    es = go.elements(c.xs, c.l2s, g0)
    exact_total = go.sumsq(np.concatenate(es))
    clip = np.float32(0.5 * math.sqrt(exact_total))
    got, _ = c.guard(dev(g0), state_tensor(clip=clip))
    n = c.total
    rel = abs(got["last_sumsq"] - exact_total) / exact_total
    print(f"total sumsq {got['last_sumsq']!r} vs fsum {exact_total!r}: relative {rel:.3e}, bound {n * 2.0 ** -53:.3e}")
    assert rel <= n * 2.0 ** -53
    for s, e in enumerate(es):
        want = go.sumsq(e)
        assert abs(got["seg_sumsq"][s] - want) <= e.size * 2.0 ** -53 * want, f"segment {s}"
    assert got["clipped"] == 1 and got["last_nonfinite"] == 0 and got["ok"] == 1
    want_scale = float(clip) / math.sqrt(exact_total)
    rel_s = abs(float(got["scale"]) - want_scale) / want_scale
    print(f"scale {got['scale']!r} vs {want_scale!r}: relative {rel_s:.3e}, bound {2.0 ** -23:.3e}")
    assert rel_s <= 2.0 ** -23
    assert abs(got["last_norm"] - math.sqrt(exact_total)) <= n * 2.0 ** -53 * math.sqrt(exact_total)


def test_state_and_partials_do_not_depend_on_the_launch_shape(hip_lib):
    c, g0 = real_case()
    g = dev(g0)
    runs = []
    for cap in (1, 2, 7, 0):
        state = state_tensor(clip=3.0, skip=1, applied=5, steps=9, norm_sum=1.25, norm_max=0.5)
        got, partials = c.guard(g, state, grid_cap=cap)
        runs.append((got.tobytes(), partials.tobytes()))
        assert got["steps"] == 10 and got["applied"] == 6
    for cap, r in zip((2, 7, 0), runs[1:]):
        assert r[0] == runs[0][0], f"state block differs between grid_cap=1 and {cap}"
        assert r[1] == runs[0][1], f"partials differ between grid_cap=1 and {cap}"


# =============================================================================================== 4. non-finite
def _plant(c, g0, k):
    """Plant the first ``k`` of five non-finite elements; returns what has to be restored in c.xs."""
    seg_mis = next(i for i in range(c.nseg) if go.MISALIGN[i % len(go.MISALIGN)] and c.lengths[i] >= 3)
    spots = [("g", 0, np.nan),                                        # the first flat element
             ("g", c.total - 1, np.inf),                              # the last flat element
             ("g", int(c.edges[1]) - 1, -np.inf),                     # segment 0 has 3 * 4096 + 5 elements: its ragged tail
             ("g", int(c.edges[seg_mis]) + 1, np.nan),                # a segment stored off a 16-byte boundary
             ("x", (0, 4100), np.inf)]                                # l2 = 0.5: x infinite, g finite
    for kind, where, val in spots[:k]:
        if kind == "g":
            g0[where] = val
        else:
            c.xs[where[0]][where[1]] = val
    return k


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("skip", [1, 0])
def test_non_finite_elements_are_counted_and_skip_is_honoured(skip, k, hip_lib):
    c = Case(go.guard_lengths(7), False, 40 + k)
    assert c.l2s[0] != 0
    tab = lr_tab()[0]
    state = state_tensor(clip=1.0, skip=skip)
    clean = ints(c.rng, c.total, -4, 4)
    before, _ = c.guard(dev(clean), state)                 # a clean step first: applied = 1, lr_t set, clipped
    assert before["ok"] == 1 and before["applied"] == 1 and before["clipped"] == 1 and before["lr_t"] == tab[0]
    g0, xs_clean = clean.copy(), [x.copy() for x in c.xs]
    planted = _plant(c, g0, k)
    c.upload()
    got, partials = c.guard(dev(g0), state)
    assert got["last_nonfinite"] == planted == int(partials["nonfinite"].sum())
    assert got["clipped"] == 0 and got["scale"].tobytes() == np.float32(1.0).tobytes()
    assert not math.isfinite(got["last_norm"]) and got["finite_steps"] == 1 and got["norm_sum"] == before["norm_sum"]
    assert got["steps"] == 2 and got["clipped_steps"] == 1
    if skip:
        assert got["ok"] == 0 and got["applied"] == 1 and got["skipped_steps"] == 1
        assert got["lr_t"].tobytes() == before["lr_t"].tobytes()
    else:
        assert got["ok"] == 1 and got["applied"] == 2 and got["skipped_steps"] == 0 and got["lr_t"] == tab[1]
    ref = go.new_state(clip=1.0, skip=bool(skip))
    go.guard(ref, xs_clean, c.l2s, clean, tab)
    go.guard(ref, c.xs, c.l2s, g0, tab)
    for key in ("ok", "clipped", "scale", "lr_t", "steps", "clipped_steps", "skipped_steps", "applied", "last_nonfinite",
                "finite_steps", "norm_sum", "norm_max"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


# =============================================================================================== 5. guarded optimizer
def _moments(rng, n):
    return reals(rng, n) * np.float32(0.1), np.abs(reals(rng, n)) * np.float32(0.01)


@pytest.mark.parametrize("nseg,real_x", [(7, True), (256, False)])
def test_guarded_with_unit_scale_is_the_unguarded_kernel(nseg, real_x, hip_lib):
    """scale = 1, ok = 1: x, m, v, g, the loss and the gaps between the segments byte for byte those of
    mvin_l2_adam_multi_dev on copies.  The loss is a float atomic per workgroup: with real-valued x the case stays at two
    workgroups (two addends onto 0 commute); with integer x every L2 term is a multiple of 1/16 and any order is exact."""
    from mvin_amd import ops
    c = Case(go.guard_lengths(nseg), real_x, 500 + nseg)
    twin = Case(go.guard_lengths(nseg), real_x, 500 + nseg)
    assert np.array_equal(c.hbuf, twin.hbuf)
    if real_x:
        assert c.total <= 2 * 4096 * 4, "case bug: more than two workgroups add into the loss"
    g0 = reals(c.rng, c.total)
    m0, v0 = _moments(c.rng, c.total)
    lr_t = np.float32(0.0123)
    state = state_tensor(ok=1, scale=1.0, lr_t=lr_t, clip=3.0, applied=4)
    state_before = host(state).copy()
    out = []
    for case, guarded in ((c, True), (twin, False)):
        g, m, v = dev(g0), dev(m0), dev(v0)
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        if guarded:
            ops.l2_adam_multi_guarded(case.segs, nseg, case.total, g, m, v, loss, True, state, B1, B2, EPS)
        else:
            ops.l2_adam_multi(case.segs, nseg, case.total, g, m, v, loss, True, 0.0, B1, B2, EPS,
                              lr_dev=dev(np.array([lr_t], np.float32)))
        out.append([host(t).copy() for t in (case.buf, m, v, g, loss)])
    for name, a, b in zip(("parameters and gaps", "m", "v", "g", "loss"), *out):
        assert a.tobytes() == b.tobytes(), f"{name} differ from mvin_l2_adam_multi_dev"
    assert not np.array_equal(out[0][0], c.hbuf)                       # ... and the step did happen
    assert host(state).tobytes() == state_before.tobytes()             # the optimizer only reads the block


def _toleranced(got, ref64, ref32, what):
    ref64 = np.asarray(ref64, np.float64)
    tol = 2e-4 * np.abs(ref64).max() + 1e-7
    own = np.abs(np.asarray(ref32, np.float64).reshape(ref64.shape) - ref64).max()
    err = np.abs(np.asarray(got, np.float64).reshape(ref64.shape) - ref64).max()
    print(f"  {what}: gpu {err / tol:.3f} of tolerance, float32 formula {own / tol:.3f}")
    assert own <= 0.25 * tol, f"{what}: case bug: the float32 formula alone is at {own / tol:.2f} of the tolerance"
    assert err <= tol, f"{what}: max abs err {err:.3e} vs tolerance {tol:.3e}"


def scaled_steps_reference(c, graws, scale, lr):
    """Three guarded steps with ``scale`` in float64 (the reference) and float32 (the formula's own error): per step the
    unscaled gradient with its L2 term and the L2 loss, at the end parameters and moments."""
    names = [str(i) for i in range(c.nseg)]
    opts = {dt: go.GuardedAdam(dict(zip(names, c.xs)), lr, B1, B2, EPS, dtype=dt) for dt in (np.float64, np.float32)}
    ps = {dt: {k: x.astype(dt) for k, x in zip(names, c.xs)} for dt in opts}
    per_step = []
    for graw in graws:
        gall, l2l = {}, {}
        for dt, opt in opts.items():
            grads = {k: graw[c.edges[i]:c.edges[i + 1]].astype(dt) + dt(np.float32(c.l2s[i])) * ps[dt][k]
                     for i, k in enumerate(names)}
            gall[dt] = np.concatenate([grads[k] for k in names])
            l2l[dt] = sum(dt(0.5) * dt(np.float32(c.l2s[i])) * (ps[dt][k] * ps[dt][k]).sum(dtype=dt)
                          for i, k in enumerate(names))
            ps[dt] = opt.step(ps[dt], grads, scale=scale)
        per_step.append((gall, l2l))
    cat = lambda d: np.concatenate([np.asarray(d[k]).ravel() for k in names])
    return per_step, {dt: (cat(ps[dt]), cat(opts[dt].m), cat(opts[dt].v)) for dt in opts}


def scaled_steps_inputs(nseg):
    c = Case(go.guard_lengths(nseg), True, 600 + nseg)
    graws = []
    for _ in range(3):
        g = reals(c.rng, c.total)
        graws.append(np.where(np.abs(g) < 1e-2, np.copysign(np.float32(1e-2), g), g).astype(np.float32))
    return c, graws


@pytest.mark.parametrize("nseg", [7, 256])
def test_guarded_three_scaled_steps_against_float64(nseg, hip_lib):
    from mvin_amd import ops
    c, graws = scaled_steps_inputs(nseg)
    scale = np.float32(0.37)
    per_step, end = scaled_steps_reference(c, graws, scale, LR)
    m = torch.zeros(c.total, dtype=torch.float32, device=DEV)
    v = torch.zeros(c.total, dtype=torch.float32, device=DEV)
    for t, graw in enumerate(graws, 1):
        lr_t = np.float32(LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t))
        state = state_tensor(ok=1, scale=scale, lr_t=lr_t)
        g, loss = dev(graw), torch.zeros(1, dtype=torch.float32, device=DEV)
        ops.l2_adam_multi_guarded(c.segs, nseg, c.total, g, m, v, loss, True, state, B1, B2, EPS)
        gall, l2l = per_step[t - 1]
        _toleranced(host(g), gall[np.float64], gall[np.float32], f"step {t} g (unscaled)")
        _toleranced(host(loss)[0], l2l[np.float64], l2l[np.float32], f"step {t} loss")
    got_p = np.concatenate(c.params())
    for got, k, name in ((got_p, 0, "parameters"), (host(m), 1, "m"), (host(v), 2, "v")):
        _toleranced(got, end[np.float64][k], end[np.float32][k], f"{name} after 3 scaled steps")


@pytest.mark.parametrize("nseg", [7, 256])
def test_guarded_with_ok_zero_writes_no_parameter_and_no_moment(nseg, hip_lib):
    from mvin_amd import ops
    c = Case(go.guard_lengths(nseg), False, 700 + nseg)
    g0 = reals(c.rng, c.total)
    m0, v0 = _moments(c.rng, c.total)
    g, m, v = dev(g0), dev(m0), dev(v0)
    loss = torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    state = state_tensor(ok=0, scale=0.5, lr_t=0.1, skip=1)
    ops.l2_adam_multi_guarded(c.segs, nseg, c.total, g, m, v, loss, True, state, B1, B2, EPS)
    assert host(c.buf).tobytes() == c.hbuf.tobytes()                   # parameters and the gaps between them
    assert host(m).tobytes() == m0.tobytes() and host(v).tobytes() == v0.tobytes()
    # g as the unguarded kernel writes it back (unscaled, L2 term added); the loss gained the L2 term: integers x, so the
    # terms are multiples of 1/16 and the float32 sum is exact in any order
    want_g = np.concatenate(go.elements(c.xs, c.l2s, g0))
    assert host(g).tobytes() == want_g.tobytes()
    l2 = sum(0.5 * c.l2s[i] * float((c.xs[i].astype(np.float64) ** 2).sum()) for i in range(nseg))
    assert l2 * 16 == round(l2 * 16) and (l2 + 3.0) * 16 < 2.0 ** 24, "case bug: the loss is not exact in float32"
    assert float(host(loss)[0]) == 3.0 + l2
    # ... and the same launch with ok = 1 does step
    state = state_tensor(ok=1, scale=0.5, lr_t=0.1)
    ops.l2_adam_multi_guarded(c.segs, nseg, c.total, dev(g0), m, v, loss, True, state, B1, B2, EPS)
    assert host(m).tobytes() != m0.tobytes() and not np.array_equal(host(c.buf), c.hbuf)
