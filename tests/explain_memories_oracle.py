"""The rule of mvin_explain_memories (include/mvin_hip.h) in numpy and plain Python.

Blocks are [h-set (when there is a w_h) | hop 0 | .. | hop P-1]; block c's memories are the Nm slots of
uts[clamp(user), hop, :, :] (hop 0 for the h-set block).  Two oracles:

(a) ``rank_oracle``: from per-slot probabilities and contributions (float32, as the kernel wrote them) to everything that is
    selection -- clean, mass = floor(double(clean(p)) * 2^40), merge by key (h, or (h, r, t); RAW stored ids), mass descending
    then slot ascending, the merged contribution and the block sum as float32 sums in ascending slot order from +0, the
    per-relation masses.  The kernel must reproduce this bit for bit.
(b) ``arith_oracle``: logits, probabilities, values, contributions, block sums and the bias term in one dtype: float64 is the
    reference, float32 (the same formulas written the plain numpy way) the yardstick a float32 kernel is measured against."""
import numpy as np

from explain_oracle import clean, mass1

SCALE = float(2 ** 40)


def block_names(P, has_set):
    return (["h_set"] if has_set else []) + [f"hop{i}" for i in range(P)]


def triples(uts, users, P, has_set):
    """RAW ids per (pair, block, slot): int32 [B, n_o, 3, Nm]; users are clamped into the table, the h-set block is hop 0."""
    uts = np.asarray(uts, np.int32)
    u = np.clip(np.asarray(users, np.int64), 0, uts.shape[0] - 1)
    hops = ([0] if has_set else []) + list(range(P))
    return uts[u][:, hops]


def f32_sum_ascending(values):
    """float32 sum in the given order, starting from +0 -- the order is part of the rule."""
    acc = np.float32(0.0)
    for v in np.asarray(values, np.float32):
        acc = np.float32(acc + v)
    return acc


def rank_oracle(probs, slot_contrib, uts, users, P, has_set, top, n_relation=None):
    """-> dict(mem int32 [B, n_o, top, 3], mass int64 / contrib f32 / slot int32 [B, n_o, top], distinct int32 / total int64 /
    block f32 [B, n_o], rel_mass int64 [P, n_relation] or None: what ONE call adds to a zeroed buffer)."""
    probs, slot_contrib = np.asarray(probs, np.float32), np.asarray(slot_contrib, np.float32)
    B, n_o, Nm = probs.shape
    trip = triples(uts, users, P, has_set)
    masses = mass1(probs)                                        # int64 [B, n_o, Nm]
    mem = np.full((B, n_o, top, 3), -1, np.int32)
    mass = np.zeros((B, n_o, top), np.int64)
    contrib = np.zeros((B, n_o, top), np.float32)
    slot = np.full((B, n_o, top), -1, np.int32)
    distinct = np.zeros((B, n_o), np.int32)
    total = masses.sum(axis=2).astype(np.int64)
    block = np.zeros((B, n_o), np.float32)
    rel_mass = None if n_relation is None else np.zeros((P, n_relation), np.int64)
    for b in range(B):
        for c in range(n_o):
            is_set = has_set and c == 0
            h, r, t = (trip[b, c, i].astype(np.int64) for i in range(3))
            keys = [(int(h[m]), -1, -1) if is_set else (int(h[m]), int(r[m]), int(t[m])) for m in range(Nm)]
            groups = {}
            for m, k in enumerate(keys):                         # ascending slot order
                groups.setdefault(k, []).append(m)
            merged = [(-int(masses[b, c, s].sum()), s[0], k, f32_sum_ascending(slot_contrib[b, c, s])) for k, s in groups.items()]
            merged.sort(key=lambda e: e[:2])                     # mass descending, then lowest slot ascending
            distinct[b, c] = len(merged)
            for row, (neg, s0, k, cs) in enumerate(merged[:top]):
                mem[b, c, row], mass[b, c, row], contrib[b, c, row], slot[b, c, row] = k, -neg, cs, s0
            block[b, c] = f32_sum_ascending(slot_contrib[b, c])
            if rel_mass is not None and not is_set:
                ok = (r >= 0) & (r < n_relation)
                np.add.at(rel_mass[c - (1 if has_set else 0)], r[ok], masses[b, c][ok])
    return dict(mem=mem, mass=mass, contrib=contrib, slot=slot, distinct=distinct, total=total, block=block, rel_mass=rel_mass)


def arith_oracle(E, V, w_h, uts, users, G, mlp_bias, item_final, P, dtype=np.float64):
    """-> dict(probs, slot_contrib, value [B, n_o, Nm], block [B, n_o], bias [B]) evaluated in ``dtype``; reads clamp entity ids
    into [0, n_entity), relation ids into [0, nR) and user ids into [0, n_user)."""
    E = np.asarray(E).astype(dtype)
    has_set = w_h is not None
    trip = triples(uts, users, P, has_set).astype(np.int64)
    B, n_o, _, Nm = trip.shape
    D = E.shape[1]
    G = np.asarray(G).astype(dtype).reshape(B, n_o, D)
    h = np.clip(trip[:, :, 0], 0, E.shape[0] - 1)
    t = np.clip(trip[:, :, 2], 0, E.shape[0] - 1)
    probs = np.zeros((B, n_o, Nm), dtype)
    value = np.zeros((B, n_o, Nm), dtype)
    for c in range(n_o):
        Eh = E[h[:, c]]                                          # [B, Nm, D]
        if has_set and c == 0:
            logit = (Eh * np.asarray(w_h).astype(dtype)[None, None, :D]).sum(axis=-1)
            x = Eh
        else:
            Vd = np.asarray(V).astype(dtype)
            r = np.clip(trip[:, c, 1], 0, Vd.shape[1] - 1)
            logit = (Eh * Vd[np.arange(B)[:, None], r]).sum(axis=-1)
            x = E[t[:, c]]
        e = np.exp(logit - logit.max(axis=-1, keepdims=True))
        probs[:, c] = e / e.sum(axis=-1, keepdims=True)
        value[:, c] = (x * G[:, c][:, None, :]).sum(axis=-1)
    slot_contrib = probs * value
    bias = (np.asarray(mlp_bias).astype(dtype)[None, :] * np.asarray(item_final).astype(dtype)).sum(axis=-1)
    return dict(probs=probs, slot_contrib=slot_contrib, value=value, block=slot_contrib.sum(axis=-1), bias=bias)
