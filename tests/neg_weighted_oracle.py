"""Host restatement of mvin_sample_negatives_weighted (TEST INFRASTRUCTURE; the rule is stated in include/mvin_hip.h).
Integer work: the GPU output must match bit for bit.

For user u: X_u = the in-range ids of its exclusion row united with the masked items (bit i % 32 of word i / 32 of ``mask``;
bits at positions >= n_item are ignored; None = nothing masked), c_u = n_item - |X_u|, m_eff = min(m[u], c_u).  Draw j takes two
words of stream 6: r0 = rnd32(seed, 6, u, round, 2j), r1 = rnd32(seed, 6, u, round, 2j + 1); bucket i = (r0 * n_item) >> 32 and
x_j = i if r1 < thresh[i] else min(alias[i], n_item - 1), for j < 64 * n_item.  The negatives are the first m_eff values of
that sequence that are not in X_u and have not occurred earlier, in sequence order; unfilled slots hold -1.

``sample_negatives_scalar`` is the literal rule with Python ints and sets; ``sample_negatives_np`` draws blocks of j with
uint64 numpy arithmetic and filters them in order (for the bigger GPU cases).  tests/test_negatives_weighted_host.py compares
the two."""
import numpy as np

from neg_oracle import M64, _assemble, _row, draw_cap
from oracle.prep_ref import rnd32

STREAM = 6


def masked_items(mask, n_item):
    """bool [n_item]: the items whose mask bit is set (``mask`` None: none)."""
    if mask is None:
        return np.zeros(n_item, dtype=bool)
    words = np.asarray(mask).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    assert words.size == (n_item + 31) // 32
    return ((words[:, None] >> np.arange(32)[None, :]) & 1).astype(bool).reshape(-1)[:n_item]


def draw_scalar(tab, n_item, seed, round, u, j):
    r0 = rnd32(seed, STREAM, u, round, 2 * j)
    r1 = rnd32(seed, STREAM, u, round, 2 * j + 1)
    i = (r0 * n_item) >> 32
    return i if r1 < int(tab[i][0]) else min(int(tab[i][1]), n_item - 1)


def user_negatives_scalar(row, m, n_item, tab, mask, seed, round, u):
    """One user: (items list of length m with -1 padding, draws consumed)."""
    X = {int(i) for i in row if 0 <= int(i) < n_item} | set(np.flatnonzero(masked_items(mask, n_item)).tolist())
    m_eff = min(m, n_item - len(X))
    if not isinstance(tab, list):
        tab = (np.asarray(tab).astype(np.int64) & 0xFFFFFFFF).tolist()
    got, seen, j = [], set(), 0
    while len(got) < m_eff and j < draw_cap(n_item):
        x = draw_scalar(tab, n_item, seed, round, u, j)
        j += 1
        if x in X or x in seen:
            continue
        seen.add(x)
        got.append(x)
    return got + [-1] * (m - len(got)), j


def sample_negatives_scalar(excl_ptr, excl_ids, counts, n_item, tab, mask=None, seed=1, round=0):
    """-> (out_ptr int64 [nU+1], out_items int32, status int64 [2] = users short, slots left at -1)."""
    counts = [int(c) for c in np.asarray(counts).tolist()]
    tab = (np.asarray(tab).astype(np.int64) & 0xFFFFFFFF).tolist()
    per_user = [user_negatives_scalar(_row(excl_ptr, excl_ids, u), m, n_item, tab, mask, seed, round, u)[0] if m > 0 else []
                for u, m in enumerate(counts)]
    return _assemble(per_user, counts)


def words_np(seed, round, u, c0, c1):
    """rnd32(seed, 6, u, round, c) for c in [c0, c1) as a uint64 array, in wrapping uint64 arithmetic."""
    head = (seed ^ (STREAM * 0xD1B54A32D192ED03) ^ (u * 0x9E3779B97F4A7C15) ^ (round * 0xC2B2AE3D27D4EB4F)) & M64
    with np.errstate(over="ignore"):
        z = np.uint64(head) ^ (np.arange(c0, c1, dtype=np.uint64) * np.uint64(0x165667B19E3779F9))
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return z >> np.uint64(32)


def draws_np(tab, n_item, seed, round, u, j0, j1):
    """x_j for j in [j0, j1) as an int64 array."""
    tab = np.asarray(tab).astype(np.int64) & 0xFFFFFFFF
    w = words_np(seed, round, u, 2 * j0, 2 * j1)
    r0, r1 = w[0::2], w[1::2].astype(np.int64)
    i = ((r0 * np.uint64(n_item)) >> np.uint64(32)).astype(np.int64)
    return np.where(r1 < tab[i, 0], i, np.minimum(tab[i, 1], n_item - 1))


def user_negatives_np(row, m, n_item, tab, mask, seed, round, u):
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    taken = masked_items(mask, n_item).copy()
    taken[row[(row >= 0) & (row < n_item)]] = True
    m_eff = min(m, n_item - int(taken.sum()))
    got, n_got, j, cap = [], 0, 0, draw_cap(n_item)
    while n_got < m_eff and j < cap:
        j1 = min(cap, j + max(1024, 2 * (m_eff - n_got)))
        x = draws_np(tab, n_item, seed, round, u, j, j1)
        x = x[~taken[x]]                                           # eligible, not drawn in an earlier block
        first = np.sort(np.unique(x, return_index=True)[1])        # first occurrences inside the block, in j order
        x = x[first][:m_eff - n_got]
        taken[x] = True
        got.append(x)
        n_got += x.size
        j = j1
    got = np.concatenate(got) if got else np.zeros(0, dtype=np.int64)
    return np.concatenate([got, np.full(m - got.size, -1, dtype=np.int64)]).astype(np.int32)


def sample_negatives_np(excl_ptr, excl_ids, counts, n_item, tab, mask=None, seed=1, round=0):
    counts = [int(c) for c in np.asarray(counts).tolist()]
    tab = np.asarray(tab).astype(np.int64) & 0xFFFFFFFF
    per_user = [user_negatives_np(_row(excl_ptr, excl_ids, u), m, n_item, tab, mask, seed, round, u).tolist() if m > 0 else []
                for u, m in enumerate(counts)]
    return _assemble(per_user, counts)
