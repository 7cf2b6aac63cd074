"""Plain Python / numpy oracle of mvin_topk_segments and mvin_rank_segments: per segment, the eligible entries in Python's stable
``sorted(key=(image, -position), reverse=True)`` -- image = a host restatement of mvin_score_image.h (-0.0 equals +0.0, every
NaN is equal and below -inf) -- and, for the queries, plain counts over the eligible entries."""
import numpy as np

MISSING_BITS = 0x7FC00000
NEG_INF_BITS = 0xFF800000


def score_image(v):
    """mvin_score_image.h for one f32 given as a numpy float32: a Python int."""
    u = int(np.float32(v).view(np.uint32))
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return 0
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _segments(scores, seg_ptr, ids, excl, max_len):
    """Per segment: (base, length or None when over the bound, eligible positions, images of all positions)."""
    scores = np.asarray(scores, np.float32)
    seg_ptr = np.asarray(seg_ptr, np.int64)
    for s in range(len(seg_ptr) - 1):
        lo, hi = int(seg_ptr[s]), int(seg_ptr[s + 1])
        if max_len is not None and hi - lo > max_len:
            yield lo, None, [], []
            continue
        ex = set() if excl is None else set(int(e) for e in excl[s])
        elig = [p for p in range(hi - lo) if ids is None or (int(ids[lo + p]) >= 0 and int(ids[lo + p]) not in ex)]
        yield lo, hi - lo, elig, [score_image(x) for x in scores[lo:hi]]


def topk_segments_oracle(scores, seg_ptr, k, ids=None, excl=None, max_len=None):
    """Returns (pos int32 [n_seg, k], value bits uint32 [n_seg, k], ids int32 [n_seg, k], status [2])."""
    bits = np.asarray(scores, np.float32).view(np.uint32)
    n_seg = len(seg_ptr) - 1
    pos = np.full((n_seg, k), -1, np.int32)
    vals = np.full((n_seg, k), NEG_INF_BITS, np.uint32)
    oid = np.full((n_seg, k), -1, np.int32)
    status = [0, 0]
    for s, (lo, length, elig, img) in enumerate(_segments(scores, seg_ptr, ids, excl, max_len)):
        if length is None:
            status[0] += 1
            status[1] += k
            continue
        best = sorted(elig, key=lambda p: (img[p], -p), reverse=True)[:k]
        for slot, p in enumerate(best):
            pos[s, slot] = p
            vals[s, slot] = bits[lo + p]
            if ids is not None:
                oid[s, slot] = ids[lo + p]
    return pos, vals, oid, status


def rank_segments_oracle(scores, seg_ptr, q_ptr, q_pos, ids=None, excl=None, max_len=None):
    """Returns (counts int32 [Q, 3], value bits uint32 [Q], eligible int32 [n_seg], status [2])."""
    bits = np.asarray(scores, np.float32).view(np.uint32)
    n_seg = len(seg_ptr) - 1
    counts = np.full((len(q_pos), 3), -1, np.int32)
    vals = np.full(len(q_pos), MISSING_BITS, np.uint32)
    eligible = np.zeros(n_seg, np.int32)
    status = [0, 0]
    for s, (lo, length, elig, img) in enumerate(_segments(scores, seg_ptr, ids, excl, max_len)):
        q0, q1 = int(q_ptr[s]), int(q_ptr[s + 1])
        if length is None:
            status[0] += 1
            status[1] += q1 - q0
            eligible[s] = -1
            continue
        eligible[s] = len(elig)
        e_pos = np.asarray(elig, np.int64)
        e_img = np.asarray([img[p] for p in elig], np.int64)
        inside = set(elig)
        for t in range(q0, q1):
            p = int(q_pos[t])
            if p not in inside:
                continue
            same = e_img == img[p]
            counts[t] = (int((e_img > img[p]).sum()), int((same & (e_pos < p)).sum()), int((same & (e_pos > p)).sum()))
            vals[t] = bits[lo + p]
    return counts, vals, eligible, status
