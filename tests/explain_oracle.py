"""The rule of mvin_explain_paths (include/mvin_hip.h) in numpy and plain Python: what the kernel must give bit for bit.

A pair's entries are its path slots s = k1 * K + k2 (one-hop mode, ``imp1 is None``: its K level-1 slots).  Weights are cleaned
(NaN, +-inf and anything <= 0 -> 0, anything above 1 -> 1), a slot's mass is the int64 floor(double(w0) * double(w1) * 2^40)
(one-hop: floor(double(w0) * 2^40)), slots with the same (rel0, ent1, rel1, ent2) merge into one path whose mass is the integer
sum and whose slot is the lowest of them, and paths are listed by mass descending, then slot ascending.  A path slot whose rel1
lies outside [0, 2^25) or whose ent2 is negative does not fit the kernel's key and is dropped: mass 0 everywhere, in no path."""
import numpy as np

SCALE = float(2 ** 40)
REL_FIELD = 1 << 25


def clean(w):
    """float32 weights -> float32 in [0, 1]: NaN, +-inf and anything <= 0 become 0, anything above 1 becomes 1."""
    w = np.asarray(w, np.float32)
    ok = np.isfinite(w) & (w > 0)
    return np.where(ok, np.minimum(np.where(ok, w, 0), np.float32(1)), np.float32(0)).astype(np.float32)


def mass1(w0):
    """int64 floor(double(w0) * 2^40) of cleaned level-1 weights."""
    return np.floor(clean(w0).astype(np.float64) * SCALE).astype(np.int64)


def mass2(w0, w1):
    """int64 floor(double(w0) * double(w1) * 2^40): the product of two floats is exact in double, and so is the scaling."""
    return np.floor(clean(w0).astype(np.float64) * clean(w1).astype(np.float64) * SCALE).astype(np.int64)


def fits(rel1, ent2):
    rel1, ent2 = np.asarray(rel1, np.int64), np.asarray(ent2, np.int64)
    return (rel1 >= 0) & (rel1 < REL_FIELD) & (ent2 >= 0)


def slot_masses(imp0, imp1, rel1=None, ent2=None):
    """[B, N] int64 masses of every entry; a path slot that does not fit the key has mass 0."""
    imp0 = np.asarray(imp0, np.float32)
    B, K = imp0.shape[0], imp0.shape[-1]
    imp0 = imp0.reshape(B, K)
    if imp1 is None:
        return mass1(imp0)
    imp1 = np.asarray(imp1, np.float32).reshape(B, K, K)
    m = mass2(imp0[:, :, None], imp1).reshape(B, K * K)
    return np.where(fits(np.asarray(rel1).reshape(B, K * K), np.asarray(ent2).reshape(B, K * K)), m, 0)


def explain_oracle(imp0, imp1, rel0, ent1, rel1, ent2, top, n_relation=None):
    """-> dict(paths int32 [B, top, 4], mass int64 [B, top], slot int32 [B, top], distinct int32 [B], total int64 [B],
    rel_mass int64 [2, n_relation] or None): one call's outputs, rel_mass as ONE call adds it to a zeroed buffer."""
    imp0 = np.asarray(imp0, np.float32)
    B, K = imp0.shape[0], imp0.shape[-1]
    two = imp1 is not None
    N = K * K if two else K
    rel0 = np.asarray(rel0, np.int32).reshape(B, K)
    ent1 = np.asarray(ent1, np.int32).reshape(B, K)
    if two:
        rel1 = np.asarray(rel1, np.int32).reshape(B, N)
        ent2 = np.asarray(ent2, np.int32).reshape(B, N)
        ok = fits(rel1, ent2)
    else:
        ok = np.ones((B, N), bool)
    masses = slot_masses(imp0, imp1, rel1, ent2)
    paths = np.full((B, top, 4), -1, np.int32)
    mass = np.zeros((B, top), np.int64)
    slot = np.full((B, top), -1, np.int32)
    distinct = np.zeros(B, np.int32)
    total = masses.sum(axis=1).astype(np.int64)
    k1 = np.arange(N) // K if two else np.arange(N)
    for b in range(B):
        s = np.flatnonzero(ok[b])                            # the slots that are entries
        if s.size == 0:
            continue
        keys = np.stack([rel0[b, k1], ent1[b, k1], rel1[b] if two else np.full(N, -1), ent2[b] if two else np.full(N, -1)],
                        axis=1).astype(np.int64)[s]
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        m = np.zeros(len(uniq), np.int64)
        np.add.at(m, inv, masses[b, s])                      # a path's mass: the integer sum over its slots
        lowest = np.full(len(uniq), N, np.int64)
        np.minimum.at(lowest, inv, s)                        # its slot: the lowest of them
        order = np.lexsort((lowest, -m))[:top]               # mass descending, then slot ascending
        distinct[b] = len(uniq)
        paths[b, :len(order)] = uniq[order]
        mass[b, :len(order)] = m[order]
        slot[b, :len(order)] = lowest[order]
    rel_mass = None
    if n_relation is not None:
        rel_mass = np.zeros((2, n_relation), np.int64)
        m0 = mass1(imp0.reshape(B, K))
        inr = (rel0 >= 0) & (rel0 < n_relation)
        np.add.at(rel_mass[0], rel0[inr], m0[inr])
        if two:
            inr = (rel1 >= 0) & (rel1 < n_relation)
            np.add.at(rel_mass[1], rel1[inr], masses[inr])
    return dict(paths=paths, mass=mass, slot=slot, distinct=distinct, total=total, rel_mass=rel_mass)
