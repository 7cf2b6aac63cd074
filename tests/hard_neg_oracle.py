"""Host oracle of mvin_select_negatives (include/mvin_hip.h states the rule): Python integers for one group
(``select_group``, on top of oracle/prep_ref.rnd32) and the same rule over many groups in numpy (``select_negatives``, with a
uint64 restatement of rnd32 that tests/test_hard_negatives_host.py pins against prep_ref.rnd32 and against ``select_group``).
Nothing here imports the library."""
import numpy as np

from oracle import prep_ref

STREAM = 5                      # csrc/mvin_rnd.h: streams in use
QNAN_BITS = 0x7FC00000


def score_image(scores):
    """csrc/mvin_score_image.h on an array of f32: the order-preserving uint32 image; -0.0 = +0.0, every NaN -> 0."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = np.where(u == 0x80000000, 0, u)
    img = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(nan, 0, img).astype(np.int64)


def rnd32_np(seed, stream, a, b, c):
    """prep_ref.rnd32 on uint64 arrays (wrapping arithmetic)."""
    u = lambda x: np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (u(seed) ^ (u(stream) * u(0xD1B54A32D192ED03)) ^ (u(a) * u(0x9E3779B97F4A7C15)) ^ (u(b) * u(0xC2B2AE3D27D4EB4F))
             ^ (u(c) * u(0x165667B19E3779F9)))
        z = z + u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(32)).astype(np.int64)


def order_a(scores_row, valid_row=None):
    """The candidate slots of one group in order A (higher score first, ties to the lower slot)."""
    img = score_image(scores_row).tolist()
    cand = [j for j in range(1, len(img)) if valid_row is None or valid_row[j] != 0]
    return sorted(cand, key=lambda j: (-img[j], j))


def select_group(scores_row, valid_row, n_neg, shortlist, seed, round, key):
    """One group in Python integers.  Returns (chosen slots in order A, the slots of order B over the shortlist)."""
    a = order_a(scores_row, valid_row)
    short = a[:min(shortlist, len(a))]
    b = sorted(short, key=lambda j: (prep_ref.rnd32(seed & prep_ref.M64, STREAM, key & prep_ref.M64, round & prep_ref.M64, j), j))
    chosen = set(b[:min(n_neg, len(short))])
    return [j for j in a if j in chosen], b


def _ranks(keys):
    """Per row: the rank of every column under ascending ``keys`` (distinct per row)."""
    order = np.argsort(keys, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(keys.shape[1]), keys.shape), axis=1)
    return rank


def select_negatives(scores, items, valid, n_neg, shortlist, seed, round, group_key=None):
    """The rule over [n, Gp] arrays.  Returns (out_items int64 [n, 1 + n_neg], out_valid f32, out_score_bits uint32,
    counts = 4 Python ints, chosen bool [n, Gp], first_b int [n]: the first slot of order B, -1 without a candidate)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    items = np.asarray(items, dtype=np.int64)
    n, Gp = scores.shape
    assert 2 <= Gp <= 64 and 1 <= n_neg <= shortlist <= Gp - 1 and items.shape == (n, Gp)
    slot = np.arange(Gp, dtype=np.int64)[None, :]
    cand = np.ones((n, Gp), dtype=bool) if valid is None else (np.asarray(valid).reshape(n, Gp) != 0)
    cand[:, 0] = False
    img = score_image(scores).reshape(n, Gp)
    BIG = np.int64(1) << 60
    rank_a = _ranks(np.where(cand, -img * 64 + slot, BIG + slot))            # candidates first, image descending, slot ascending
    in_s = cand & (rank_a < shortlist)
    key = np.arange(n, dtype=np.uint64) if group_key is None else np.asarray(group_key).astype(np.uint64)
    r = rnd32_np(np.uint64(seed & prep_ref.M64), STREAM, key[:, None], np.uint64(round & prep_ref.M64), slot.astype(np.uint64))
    rank_b = _ranks(np.where(in_s, r * 64 + slot, BIG + slot))
    chosen = in_s & (rank_b < n_neg)
    place = 1 + _ranks(np.where(chosen, rank_a, BIG + slot))                 # the chosen, hardest first
    Go = 1 + n_neg
    out_items = np.repeat(items[:, :1], Go, axis=1)
    out_valid = np.zeros((n, Go), dtype=np.float32)
    out_bits = np.full((n, Go), QNAN_BITS, dtype=np.uint32)
    bits = scores.view(np.uint32)
    out_valid[:, 0] = 1.0
    out_bits[:, 0] = bits[:, 0]
    g, j = np.nonzero(chosen)
    out_items[g, place[g, j]] = items[g, j]
    out_valid[g, place[g, j]] = 1.0
    out_bits[g, place[g, j]] = bits[g, j]
    gt, eq = img > img[:, :1], img == img[:, :1]
    counts = (int((2 * (gt & chosen) + (eq & chosen)).sum()), int(chosen.sum()),
              int((2 * (gt & cand) + (eq & cand)).sum()), int(cand.sum()))
    first_b = np.where(in_s.any(axis=1), np.argmin(np.where(in_s, rank_b, BIG), axis=1), -1)
    return out_items, out_valid, out_bits, counts, chosen, first_b
