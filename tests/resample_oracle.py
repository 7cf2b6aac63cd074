"""Not a test: the rule of mvin_resample_sums (include/mvin_hip.h) restated in numpy, bit for bit, and an order-free reference.

  draws(mode, seed, n_rows, reps)          the row i and the sign s of every (replicate, position)
  resample_sums(vals, mode, seed, reps)    the rule: 64 strided partial sums accumulated in ascending j, then the halving tree
  resample_fsum(vals, mode, seed, reps)    math.fsum per (replicate, column) over the same draws: exact up to one rounding
  gamma(n)                                 n u / (1 - n u), u = 2^-53: the bound of any summation order of n terms

The hash is csrc/mvin_rnd.h's rnd32 in uint64 arithmetic (numpy wraps modulo 2^64, like the device), as oracle/prep_ref.py
restates it in Python integers."""
import math

import numpy as np

MODES = {"bootstrap": 0, "signflip": 1, "observed": 2}
ROW_STREAM, SIGN_STREAM = 7, 8
U64 = np.uint64


def rnd32(seed, stream, a, b, c):
    """rnd32(seed, stream, a, b, c) for arrays (or scalars) a, b, c: uint64 in, uint64 holding a 32-bit word out."""
    with np.errstate(over="ignore"):
        z = (U64(seed & 0xFFFFFFFFFFFFFFFF) ^ (U64(stream) * U64(0xD1B54A32D192ED03)) ^ (np.asarray(a, U64) * U64(0x9E3779B97F4A7C15))
             ^ (np.asarray(b, U64) * U64(0xC2B2AE3D27D4EB4F)) ^ (np.asarray(c, U64) * U64(0x165667B19E3779F9)))
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z = z ^ (z >> U64(31))
    return z >> U64(32)


def draws(mode, seed, n_rows, reps):
    """(rows int64 [R, n_rows], signs f64 [R, n_rows]) of the replicates ``reps`` (any iterable of replicate numbers)."""
    mode = MODES.get(mode, mode)
    reps = np.asarray(list(reps), dtype=np.uint64).reshape(-1, 1)
    j = np.arange(n_rows, dtype=np.uint64).reshape(1, -1)
    rows = np.broadcast_to(j.astype(np.int64), (reps.size, n_rows)).copy()
    signs = np.ones((reps.size, n_rows), dtype=np.float64)
    if mode == 0:
        rows = ((rnd32(seed, ROW_STREAM, reps, 0, j) * U64(n_rows)) >> U64(32)).astype(np.int64)
    elif mode == 1:
        signs = np.where((rnd32(seed, SIGN_STREAM, reps, 0, j) >> U64(31)) != 0, -1.0, 1.0)
    elif mode != 2:
        raise ValueError(f"mode={mode}")
    return rows, signs


def _terms(vals, mode, seed, reps):
    """s * x per (replicate, position, column), f64 [R, n_rows, n_cols] (NaN where the cell is NaN)."""
    vals = np.asarray(vals, dtype=np.float64)
    rows, signs = draws(mode, seed, vals.shape[0], reps)
    return vals[rows] * signs[:, :, None]


def resample_sums(vals, mode, seed, reps):
    """The rule: (sums f64 [R, n_cols], counts int32 [R, n_cols])."""
    t = _terms(vals, mode, seed, reps)
    R, U, M = t.shape
    ok = ~np.isnan(t)
    p = np.zeros((R, 64, M), dtype=np.float64)
    n = np.zeros((R, 64, M), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(0, U, 64):                                  # ascending j: p_l += s x for l = j mod 64
            w = min(64, U - b)
            p[:, :w] = np.where(ok[:, b:b + w], p[:, :w] + t[:, b:b + w], p[:, :w])
            n[:, :w] += ok[:, b:b + w]
        h = 32
        while h >= 1:
            p[:, :h] = p[:, :h] + p[:, h:2 * h]
            h //= 2
    return p[:, 0].copy(), n.sum(axis=1).astype(np.int32)


def resample_fsum(vals, mode, seed, reps):
    """Order-free: math.fsum per (replicate, column) of the finite-or-infinite terms; (sums, counts, abs sums)."""
    t = _terms(vals, mode, seed, reps)
    R, U, M = t.shape
    sums, asum = np.zeros((R, M)), np.zeros((R, M))
    counts = np.zeros((R, M), dtype=np.int32)
    for r in range(R):
        for c in range(M):
            x = t[r, :, c]
            x = x[~np.isnan(x)]
            counts[r, c] = x.size
            sums[r, c] = math.fsum(x.tolist()) if np.isfinite(x).all() else np.sum(x)
            asum[r, c] = math.fsum(np.abs(x).tolist()) if np.isfinite(x).all() else np.inf
    return sums, counts, asum


def gamma(n):
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


def same_bits(a, b):
    """Equal f64 bits, any NaN equal to any NaN (an inf - inf sum's sign and payload are not part of the rule)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a.view(np.uint64)[~nan] == b.view(np.uint64)[~nan]).all())
