"""Host restatement of the negative samplers' rule (TEST INFRASTRUCTURE; the rule is stated in include/mvin_hip.h).  Integer
work: the GPU output must match bit for bit.  This module owns the rule and mvin_sample_negatives' uniform draw;
tests/neg_weighted_oracle.py adds the alias draw and the mask of mvin_sample_negatives_weighted.

For user u with ineligible set X_u (the ids of its exclusion row inside [0, n_item), and the masked items if there is a mask),
c_u = n_item - |X_u| and m_eff = min(m[u], c_u): given a draw sequence x_j, j = 0, 1, ... < 64 * n_item, the negatives are the
first m_eff values of it that are not in X_u and have not occurred earlier, in sequence order; unfilled slots hold -1
(``first_eligible_scalar``: the literal rule with Python sets; ``first_eligible_np``: blocks of j filtered in order with numpy, for
the bigger GPU cases).  The uniform draw is x_j = rnd_below(n_item, seed, 4, u, round, j).  tests/test_negatives_host.py compares
``sample_negatives_scalar`` with ``sample_negatives_np``.

``round_half_up_counts`` is NegativeSampler's count rule: m[u] = floor(ratio * positives + 0.5) in float64."""
import numpy as np

from oracle.prep_ref import rnd_below

STREAM = 4
M64 = (1 << 64) - 1


def draw_cap(n_item):
    return 64 * n_item


def _row(excl_ptr, excl_ids, u):
    if excl_ptr is None:
        return []
    return np.asarray(excl_ids[int(excl_ptr[u]):int(excl_ptr[u + 1])]).tolist()


def ineligible(row, n_item, masked=None):
    """bool [n_item]: the in-range ids of ``row``, united with ``masked`` (bool [n_item]) if given."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    taken = np.zeros(n_item, dtype=bool) if masked is None else np.array(masked, dtype=bool)
    taken[row[(row >= 0) & (row < n_item)]] = True
    return taken


def first_eligible_scalar(draw, taken, m, n_item):
    """The rule for one user, draw(j) -> x_j: (items list of length m with -1 padding, draws consumed)."""
    X = set(np.flatnonzero(taken).tolist())
    m_eff = min(m, n_item - len(X))
    got, seen, j = [], set(), 0
    while len(got) < m_eff and j < draw_cap(n_item):
        x = draw(j)
        j += 1
        if x in X or x in seen:
            continue
        seen.add(x)
        got.append(x)
    return got + [-1] * (m - len(got)), j


def first_eligible_np(draws, taken, m, n_item):
    """The rule for one user, draws(j0, j1) -> integer array of x_j, j in [j0, j1): int32 [m] with -1 padding."""
    taken = taken.copy()
    m_eff = min(m, n_item - int(taken.sum()))
    got, n_got, j, cap = [], 0, 0, draw_cap(n_item)
    while n_got < m_eff and j < cap:
        j1 = min(cap, j + max(1024, 2 * (m_eff - n_got)))
        x = np.asarray(draws(j, j1)).astype(np.int64)
        x = x[~taken[x]]                                           # eligible, not drawn in an earlier block
        first = np.sort(np.unique(x, return_index=True)[1])        # first occurrences inside the block, in j order
        x = x[first][:m_eff - n_got]
        taken[x] = True
        got.append(x)
        n_got += x.size
        j = j1
    got = np.concatenate(got) if got else np.zeros(0, dtype=np.int64)
    return np.concatenate([got, np.full(m - got.size, -1, dtype=np.int64)]).astype(np.int32)


def _assemble(per_user, counts):
    out_ptr = np.zeros(len(counts) + 1, dtype=np.int64)
    out_ptr[1:] = np.cumsum(counts)
    items = np.array([x for row in per_user for x in row], dtype=np.int32).reshape(-1)
    status = np.array([sum(1 for row in per_user if -1 in row), sum(row.count(-1) for row in per_user)], dtype=np.int64)
    return out_ptr, items, status


def sample_all(one_user, excl_ptr, excl_ids, counts):
    """one_user(row, m, u) -> the m slots of user u, for every user with m > 0
    -> (out_ptr int64 [nU+1], out_items int32, status int64 [2] = users short, slots left at -1)."""
    counts = [int(c) for c in np.asarray(counts).tolist()]
    per_user = [list(one_user(_row(excl_ptr, excl_ids, u), m, u)) if m > 0 else [] for u, m in enumerate(counts)]
    return _assemble(per_user, counts)


def words_np(stream, seed, round, u, c0, c1):
    """rnd32(seed, stream, u, round, c) for c in [c0, c1) as a uint64 array, in wrapping uint64 arithmetic."""
    head = (seed ^ (stream * 0xD1B54A32D192ED03) ^ (u * 0x9E3779B97F4A7C15) ^ (round * 0xC2B2AE3D27D4EB4F)) & M64
    with np.errstate(over="ignore"):
        z = np.uint64(head) ^ (np.arange(c0, c1, dtype=np.uint64) * np.uint64(0x165667B19E3779F9))
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return z >> np.uint64(32)


# ---- the uniform draw
def user_negatives_scalar(row, m, n_item, seed, round, u):
    """One user: (items list of length m with -1 padding, draws consumed)."""
    return first_eligible_scalar(lambda j: rnd_below(n_item, seed, STREAM, u, round, j), ineligible(row, n_item), m, n_item)


def sample_negatives_scalar(excl_ptr, excl_ids, counts, n_item, seed=1, round=0):
    return sample_all(lambda row, m, u: user_negatives_scalar(row, m, n_item, seed, round, u)[0], excl_ptr, excl_ids, counts)


def draws_np(n_item, seed, round, u, j0, j1):
    """x_j for j in [j0, j1) as a uint64 array: rnd_below(n_item, seed, 4, u, round, j)."""
    return (words_np(STREAM, seed, round, u, j0, j1) * np.uint64(n_item)) >> np.uint64(32)


def user_negatives_np(row, m, n_item, seed, round, u):
    return first_eligible_np(lambda j0, j1: draws_np(n_item, seed, round, u, j0, j1), ineligible(row, n_item), m, n_item)


def sample_negatives_np(excl_ptr, excl_ids, counts, n_item, seed=1, round=0):
    return sample_all(lambda row, m, u: user_negatives_np(row, m, n_item, seed, round, u).tolist(), excl_ptr, excl_ids, counts)


def round_half_up_counts(positives_per_user, ratio):
    return np.floor(float(ratio) * np.asarray(positives_per_user, dtype=np.float64) + 0.5).astype(np.int64)
