"""Host restatement of the training-step guard (TEST INFRASTRUCTURE): include/mvin_hip.h mvin_grad_guard and
mvin_l2_adam_multi_guarded in numpy / math.fsum, independent of mvin_amd.

  elements     e = fmaf(l2, x, g) in float32 where l2 != 0, else g -- ONE rounding, as the kernels' fmaf;
  sumsq        sum of e^2: each square is exact in float64 (24-bit significand squared), math.fsum adds them with one
               rounding, so the value is the correctly rounded exact sum;
  decide       ok / clipped / scale / step size and every counter of the state block, from the rule in the header;
  lr_table     float32(lr_t(t)), t = 1..T, T = the first t with beta1**t and beta2**t both below 2**-54;
  GuardedAdam  oracle/train_ref.AdamRef (float64 by default) stepping on grads * scale, or not at all.
"""
import math

import numpy as np

from oracle import train_ref

MAX_SEG = 256
MAX_ITEM = 4096
LR_TABLE_MAX = 1 << 20


def fmaf32(a, x, g):
    """float32(a * x + g) with ONE rounding, elementwise, for float32 inputs.  The product of two float32 is exact in
    float64; its sum with g is rounded to odd in float64 (two-sum gives the rounding error's sign), and rounding a
    53-bit round-to-odd value to 24 bits is the correct rounding of the exact sum."""
    a, x, g = (np.asarray(v, np.float32).astype(np.float64) for v in (a, x, g))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * x
        s = p + g
        bb = s - p
        err = (p - (s - bb)) + (g - bb)                     # exact: s + err == p + g
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def elements(xs, l2s, g):
    """Per segment, the float32 elements the optimizer sees: xs[s] parameters, l2s[s] coefficient, g the flat gradient."""
    out, off = [], 0
    for x, l2 in zip(xs, l2s):
        x = np.asarray(x, np.float32).ravel()
        gs = np.asarray(g, np.float32).ravel()[off:off + x.size]
        l2 = np.float32(l2)
        out.append(fmaf32(l2, x, gs) if l2 != 0 else gs.copy())
        off += x.size
    return out


def sumsq(e):
    """Correctly rounded sum of squares of a float32 array (nan / inf propagate as in any IEEE sum)."""
    e = np.asarray(e, np.float32).astype(np.float64)
    if not np.all(np.isfinite(e)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float((e * e).sum())
    return math.fsum((e * e).tolist())


def count_nonfinite(e):
    return int((~np.isfinite(np.asarray(e, np.float32))).sum())


def new_state(clip=None, skip=False, applied=0):
    """The state block as a dict with the field names of mvin_guard_state."""
    return {"clip": np.float32(np.inf if clip is None else clip), "skip": int(bool(skip)), "ok": 0, "clipped": 0,
            "scale": np.float32(0.0), "lr_t": np.float32(0.0), "steps": 0, "clipped_steps": 0, "skipped_steps": 0,
            "applied": int(applied), "last_nonfinite": 0, "finite_steps": 0, "norm_sum": 0.0, "norm_max": 0.0,
            "last_norm": 0.0, "last_sumsq": 0.0, "seg_sumsq": np.zeros(MAX_SEG, np.float64)}


def decide(state, total_sumsq, nonfinite, lr_tab, seg_sumsq=None):
    """One guarded step's decision and counters, in place on ``state`` (and returned)."""
    st = state
    clip = float(np.float32(st["clip"]))
    ok = not (st["skip"] and nonfinite > 0)
    clipped = nonfinite == 0 and total_sumsq > clip * clip
    norm = math.sqrt(total_sumsq) if total_sumsq == total_sumsq and total_sumsq >= 0 else float("nan")
    st["ok"], st["clipped"] = int(ok), int(clipped)
    st["scale"] = np.float32(clip / norm) if clipped else np.float32(1.0)
    st["steps"] += 1
    st["clipped_steps"] += int(clipped)
    if ok:
        st["applied"] += 1
        st["lr_t"] = np.float32(lr_tab[min(st["applied"], len(lr_tab)) - 1])
    else:
        st["skipped_steps"] += 1
    st["last_nonfinite"] = int(nonfinite)
    st["last_sumsq"], st["last_norm"] = total_sumsq, norm
    if math.isfinite(norm):
        st["finite_steps"] += 1
        st["norm_sum"] += norm
        st["norm_max"] = max(st["norm_max"], norm)
    if seg_sumsq is not None:
        st["seg_sumsq"] = np.zeros(MAX_SEG, np.float64)
        st["seg_sumsq"][:len(seg_sumsq)] = seg_sumsq
    return st


def guard(state, xs, l2s, g, lr_tab):
    """mvin_grad_guard on host arrays: per-segment and total exact sums, the count, the decision."""
    es = elements(xs, l2s, g)
    segs = [sumsq(e) for e in es]
    flat = np.concatenate(es) if es else np.zeros(0, np.float32)
    return decide(state, sumsq(flat), count_nonfinite(flat), lr_tab, segs)


def lr_t(lr, b1, b2, t):
    """tf.train.AdamOptimizer's bias-corrected step size, betas as float32 values (what the kernels receive)."""
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def lr_table_len(b1, b2):
    """First t at which b1**t and b2**t (float32 betas) are both below 2**-54, by counting; ValueError past 2**20."""
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    lim, t = 2.0 ** -54, 1
    while b1 ** t >= lim or b2 ** t >= lim:
        t += 1
        if t > LR_TABLE_MAX:
            raise ValueError("the step-size table would need more than 2**20 entries")
    return t


def lr_table(lr, b1=0.9, b2=0.999):
    return np.array([np.float32(lr_t(lr, b1, b2, t)) for t in range(1, lr_table_len(b1, b2) + 1)], dtype=np.float32)


def work_items_ok(items, segments):
    """The work-table contract: ``items`` (records with seg / len / first) tile [0, total) exactly once in order, none
    leaves its segment (``segments`` = [(off, n)]), none is longer than MAX_ITEM or empty, and there are at most
    total / MAX_ITEM + nseg of them.  Returns None or the first violation as a string."""
    total = sum(n for _, n in segments)
    pos, last_seg = 0, -1
    for i, it in enumerate(items):
        s, ln, first = int(it["seg"]), int(it["len"]), int(it["first"])
        if not 0 <= s < len(segments) or s < last_seg:
            return f"item {i}: segment {s} out of range or descending"
        off, n = segments[s]
        if first != pos:
            return f"item {i}: starts at {first}, expected {pos}"
        if not 1 <= ln <= MAX_ITEM:
            return f"item {i}: length {ln}"
        if first < off or first + ln > off + n:
            return f"item {i}: [{first}, {first + ln}) leaves segment {s} = [{off}, {off + n})"
        pos, last_seg = first + ln, s
    if pos != total:
        return f"the items end at {pos}, total = {total}"
    if len(items) > total / MAX_ITEM + len(segments):
        return f"{len(items)} items for total = {total}, nseg = {len(segments)}"
    return None


class GuardedAdam(train_ref.AdamRef):
    """AdamRef under the guard: ``step(params, grads, scale, ok)`` applies Adam to grads * scale (scale a float32 value,
    the product rounded in this optimizer's dtype) or, with ok false, changes nothing -- not even the step count."""

    def __init__(self, params, lr, beta1=0.9, beta2=0.999, eps=1e-8, dtype=np.float64):
        super().__init__(params, lr, beta1, beta2, eps, dtype=dtype)

    def step(self, params, grads, scale=1.0, ok=True):
        if not ok:
            return params
        sc = self.dt(np.float32(scale))
        return super().step(params, {k: (np.asarray(g).astype(self.dt) * sc).astype(self.dt) for k, g in grads.items()})


# --------------------------------------------------------------------------- shapes shared by the guard's test modules
L2_CYCLE = (0.5, 0.0, 2.0, 0.25)
MISALIGN = (0, 1, 0, 3, 2)            # float offsets off a 16-byte boundary for some segments


def guard_lengths(nseg, seed=0):
    """Segment lengths of the kernel tests: multiples of 4 mixed with 1, 3, 5, 4095, 4096, 4097 and 3 * 4096 + 5."""
    base = [3 * MAX_ITEM + 5, 3, MAX_ITEM, 5, MAX_ITEM + 1, 1, MAX_ITEM - 1]
    if nseg <= len(base):
        return base[:nseg]
    rng = np.random.default_rng(seed)
    rest = [int(v) for v in rng.integers(1, 41, nseg - len(base))]
    rest[::3] = [4 * ((v + 3) // 4) for v in rest[::3]]
    return base + rest


def segments_of(lengths):
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return [(int(o), int(n)) for o, n in zip(offs[:-1], lengths)]
