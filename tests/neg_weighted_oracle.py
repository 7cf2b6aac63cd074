"""Host restatement of mvin_sample_negatives_weighted (TEST INFRASTRUCTURE; the rule is stated in include/mvin_hip.h).
Integer work: the GPU output must match bit for bit.  The rule itself -- the first m_eff eligible first occurrences of a draw
sequence -- is tests/neg_oracle.py's; this module adds what the weighted call adds to it.

The mask: X_u = the in-range ids of the exclusion row united with the masked items (bit i % 32 of word i / 32 of ``mask``; bits at
positions >= n_item are ignored; None = nothing masked).  The alias draw: draw j takes two words of stream 6,
r0 = rnd32(seed, 6, u, round, 2j), r1 = rnd32(seed, 6, u, round, 2j + 1); bucket i = (r0 * n_item) >> 32 and
x_j = i if r1 < thresh[i] else min(alias[i], n_item - 1).

``sample_negatives_scalar`` is the literal rule with Python ints and sets; ``sample_negatives_np`` draws blocks of j with
uint64 numpy arithmetic (for the bigger GPU cases).  tests/test_negatives_weighted_host.py compares the two."""
import numpy as np

import neg_oracle as no
from oracle.prep_ref import rnd32

STREAM = 6


def masked_items(mask, n_item):
    """bool [n_item]: the items whose mask bit is set (``mask`` None: none)."""
    if mask is None:
        return np.zeros(n_item, dtype=bool)
    words = np.asarray(mask).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    assert words.size == (n_item + 31) // 32
    return ((words[:, None] >> np.arange(32)[None, :]) & 1).astype(bool).reshape(-1)[:n_item]


def _u32(tab):
    return np.asarray(tab).astype(np.int64) & 0xFFFFFFFF


def draw_scalar(tab, n_item, seed, round, u, j):
    r0 = rnd32(seed, STREAM, u, round, 2 * j)
    r1 = rnd32(seed, STREAM, u, round, 2 * j + 1)
    i = (r0 * n_item) >> 32
    return i if r1 < int(tab[i][0]) else min(int(tab[i][1]), n_item - 1)


def user_negatives_scalar(row, m, n_item, tab, mask, seed, round, u):
    """One user: (items list of length m with -1 padding, draws consumed)."""
    if not isinstance(tab, list):
        tab = _u32(tab).tolist()
    return no.first_eligible_scalar(lambda j: draw_scalar(tab, n_item, seed, round, u, j),
                                    no.ineligible(row, n_item, masked_items(mask, n_item)), m, n_item)


def sample_negatives_scalar(excl_ptr, excl_ids, counts, n_item, tab, mask=None, seed=1, round=0):
    """-> (out_ptr int64 [nU+1], out_items int32, status int64 [2] = users short, slots left at -1)."""
    tab = _u32(tab).tolist()
    return no.sample_all(lambda row, m, u: user_negatives_scalar(row, m, n_item, tab, mask, seed, round, u)[0],
                         excl_ptr, excl_ids, counts)


def words_np(seed, round, u, c0, c1):
    """rnd32(seed, 6, u, round, c) for c in [c0, c1) as a uint64 array."""
    return no.words_np(STREAM, seed, round, u, c0, c1)


def draws_np(tab, n_item, seed, round, u, j0, j1):
    """x_j for j in [j0, j1) as an int64 array."""
    tab = _u32(tab)
    w = words_np(seed, round, u, 2 * j0, 2 * j1)
    r0, r1 = w[0::2], w[1::2].astype(np.int64)
    i = ((r0 * np.uint64(n_item)) >> np.uint64(32)).astype(np.int64)
    return np.where(r1 < tab[i, 0], i, np.minimum(tab[i, 1], n_item - 1))


def user_negatives_np(row, m, n_item, tab, mask, seed, round, u):
    return no.first_eligible_np(lambda j0, j1: draws_np(tab, n_item, seed, round, u, j0, j1),
                                no.ineligible(row, n_item, masked_items(mask, n_item)), m, n_item)


def sample_negatives_np(excl_ptr, excl_ids, counts, n_item, tab, mask=None, seed=1, round=0):
    tab = _u32(tab)
    return no.sample_all(lambda row, m, u: user_negatives_np(row, m, n_item, tab, mask, seed, round, u).tolist(),
                         excl_ptr, excl_ids, counts)
