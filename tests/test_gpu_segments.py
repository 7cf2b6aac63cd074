"""-m gpu: ranking inside per-user candidate lists.  mvin_topk_segments / mvin_rank_segments against the plain-Python oracle of
tests/segments_oracle.py (every comparison exact: positions, ids, counts and the input bits of the values) in the wave form and
the block form, their independence of form and max_len, their agreement with mvin_topk_rows / mvin_rank_positives, a broken
length bound, and DeviceFeeder.recommend_lists / rank_lists end to end."""
import numpy as np
import pytest
import torch

from mvin_amd import ops
from segments_oracle import rank_segments_oracle, topk_segments_oracle
from test_gpu_topk import bits, build_model, csr, make_excl, make_rows, records

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 5, 64, 1024)
GUARD = 64                                     # elements planted before and after every output buffer


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_case(lengths, seed, long_excl=False):
    """Segments of the given lengths.  Scores: four distinct values, so that ties dominate, with NaN, +-inf and +-0 planted;
    ids: distinct inside a segment, about one in nine -1; exclusion rows by turns empty, three ids of the segment and (with
    ``long_excl``, for the longest segment) more than kTopkExclLds = 2 048 ids; queries by turns none, one, every position,
    and every position plus one beyond the segment's end."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(lengths) + 1, np.int64)
    ptr[1:] = np.cumsum(lengths)
    T = int(ptr[-1])
    scores = rng.choice(np.float32([0.25, -1.5, 3.0, 0.7]), T)
    special = np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0])
    where = rng.choice(T, T // 6, replace=False)
    scores[where] = special[rng.integers(0, len(special), len(where))]
    ids = np.concatenate([rng.permutation(3 * n + 5)[:n] for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    ids[rng.random(T) < 0.11] = -1
    excl, q_rows = [], []
    for s, n in enumerate(lengths):
        own = ids[ptr[s]:ptr[s + 1]]
        own = own[own >= 0]
        if long_excl and n == max(lengths):
            row = set(rng.choice(own, min(len(own), 2100), replace=False).tolist()) | set(range(10 ** 6, 10 ** 6 + 300))
            assert len(row) > 2048
        elif s % 2 == 1 and len(own):
            row = set(rng.choice(own, min(len(own), 2), replace=False).tolist()) | {10 ** 6 + s}
        else:
            row = set()
        excl.append(row)
        q_rows.append([[], [int(rng.integers(0, max(n, 1)))], list(range(n)), list(range(n + 1))][s % 4])
    q_ptr = np.zeros(len(lengths) + 1, np.int64)
    q_ptr[1:] = np.cumsum([len(q) for q in q_rows])
    q_pos = np.asarray([p for q in q_rows for p in q], np.int32)
    return dict(ptr=ptr, scores=scores, ids=ids, excl=excl, q_ptr=q_ptr, q_pos=q_pos)


def guarded(shape, dtype):
    """An output tensor inside a larger allocation whose GUARD elements on either side hold a pattern."""
    n = int(np.prod(shape)) * (torch.empty(0, dtype=dtype).element_size() // 4)        # in 32-bit words
    whole = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    return whole[GUARD:GUARD + n].view(dtype).view(shape), whole


def guards_intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == 0x5A5A5A5A).all() and (w[-GUARD:] == 0x5A5A5A5A).all())


def run_topk(case, k, use_ids=True, use_excl=True, **kw):
    n_seg = len(case["ptr"]) - 1
    outs = [guarded((n_seg, k), torch.int32), guarded((n_seg, k), torch.float32), guarded((n_seg, k), torch.int32),
            guarded((2,), torch.int64)]
    outs[3][0].zero_()
    got = ops.topk_segments(dev(case["scores"]), dev(case["ptr"]), k, ids=dev(case["ids"]) if use_ids else None,
                            excl=csr(case["excl"]) if use_excl and use_ids else None,
                            out=(outs[0][0], outs[1][0], outs[2][0] if use_ids else None, outs[3][0]), **kw)
    torch.cuda.synchronize()
    assert all(guards_intact(w) for _, w in outs), "a write outside an output buffer"
    pos, vals, oid, status = got
    return (pos.cpu().numpy(), bits(vals.cpu().numpy()), None if oid is None else oid.cpu().numpy(), status.cpu().tolist())


def run_rank(case, use_ids=True, use_excl=True, **kw):
    n_seg, Q = len(case["ptr"]) - 1, len(case["q_pos"])
    outs = [guarded((Q, 3), torch.int32), guarded((Q,), torch.float32), guarded((n_seg,), torch.int32), guarded((2,), torch.int64)]
    outs[3][0].zero_()
    got = ops.rank_segments(dev(case["scores"]), dev(case["ptr"]), (dev(case["q_ptr"]), dev(case["q_pos"])),
                            ids=dev(case["ids"]) if use_ids else None, excl=csr(case["excl"]) if use_excl and use_ids else None,
                            out=tuple(o for o, _ in outs), **kw)
    torch.cuda.synchronize()
    assert all(guards_intact(w) for _, w in outs), "a write outside an output buffer"
    counts, vals, eligible, status = got
    return counts.cpu().numpy(), bits(vals.cpu().numpy()), eligible.cpu().numpy(), status.cpu().tolist()


def want_topk(case, k, use_ids=True, use_excl=True, max_len=None):
    pos, vals, oid, status = topk_segments_oracle(case["scores"], case["ptr"], k, ids=case["ids"] if use_ids else None,
                                                  excl=case["excl"] if use_excl and use_ids else None, max_len=max_len)
    return pos, vals, oid if use_ids else None, status


def want_rank(case, use_ids=True, use_excl=True, max_len=None):
    return rank_segments_oracle(case["scores"], case["ptr"], case["q_ptr"], case["q_pos"], ids=case["ids"] if use_ids else None,
                                excl=case["excl"] if use_excl and use_ids else None, max_len=max_len)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            np.testing.assert_array_equal(np.asarray(g), np.asarray(w))


_CASES = {}


def case_of(which):
    """The two calls of the oracle test, built once: "wave" (every length up to the cap) and "block" (those and longer ones),
    with their oracle results at the largest k (a smaller k is a prefix) and for the queries."""
    if which not in _CASES:
        cap = ops.segments_wave_cap()
        lengths = [0, 1, 2, 63, 64, 65, cap - 1, cap] + ([cap + 1, 1025, 5000] if which == "block" else [])
        case = make_case(lengths, seed=11 if which == "wave" else 12, long_excl=which == "block")
        _CASES[which] = (case, want_topk(case, max(KS)), want_rank(case), want_topk(case, max(KS), use_ids=False),
                         want_rank(case, use_ids=False))
    return _CASES[which]


def prefix(want, k):
    pos, vals, oid, status = want
    return pos[:, :k], vals[:, :k], None if oid is None else oid[:, :k], status


@pytest.mark.parametrize("which", ["wave", "block"])
def test_segments_match_oracle(hip_lib, which):
    cap = ops.segments_wave_cap()
    assert 64 <= cap <= 1024
    case, w_topk, w_rank, w_topk_plain, w_rank_plain = case_of(which)
    assert (max(np.diff(case["ptr"])) <= cap) == (which == "wave")         # the automatic form is the one the name says
    for k in KS:
        same(run_topk(case, k), prefix(w_topk, k))
    same(run_topk(case, 64, use_ids=False), prefix(w_topk_plain, 64))
    same(run_topk(case, 5, use_excl=False), want_topk(case, 5, use_excl=False))
    same(run_rank(case), w_rank)
    same(run_rank(case, use_ids=False), w_rank_plain)
    same(run_rank(case, use_excl=False), want_rank(case, use_excl=False))
    assert w_rank[0].min() == -1 and w_rank[0].max() > 0 and w_topk[0].min() == -1      # the case has missing queries and short segments


def test_segments_do_not_depend_on_form_or_bound(hip_lib):
    cap = ops.segments_wave_cap()
    case, w_topk, w_rank, _, _ = case_of("wave")
    exact = int(np.diff(case["ptr"]).max())
    assert exact == cap
    for k in (5, 1024):
        ref = run_topk(case, k, form="wave", max_len=cap)
        same(ref, prefix(w_topk, k))
        for kw in (dict(form="block", max_len=cap), dict(max_len=cap), dict(max_len=10 * cap), dict(max_len=exact), dict(),
                   dict(form="block", max_len=(1 << 31) - 1)):
            same(run_topk(case, k, **kw), ref)
    ref = run_rank(case, form="wave", max_len=cap)
    same(ref, w_rank)
    for kw in (dict(form="block", max_len=cap), dict(max_len=cap), dict(max_len=10 * cap), dict(max_len=exact), dict(),
               dict(form="block", max_len=(1 << 31) - 1)):
        same(run_rank(case, **kw), ref)
    # every lane-group width of the wave form: the same short segments under growing bounds
    short = make_case([0, 1, 2, 3, 5, 8, 7, 8, 4, 6], seed=13)
    ref_t, ref_r = want_topk(short, 5), want_rank(short)
    for bound in (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, cap):
        same(run_topk(short, 5, form="wave", max_len=bound), ref_t)
        same(run_rank(short, form="wave", max_len=bound), ref_r)
    with pytest.raises(Exception, match="form=1"):
        ops.topk_segments(dev(short["scores"]), dev(short["ptr"]), 5, form="wave", max_len=cap + 1)


def test_segments_agree_with_row_kernels(hip_lib):
    cap = ops.segments_wave_cap()
    for n in (100, cap + 7):
        seed = 40 + n
        host = make_rows(n, seed)                                               # five rows: random, ties, all equal, specials, random
        rows = host.shape[0]
        ids = (np.random.default_rng(seed).permutation(3 * n) + 11).astype(np.int64)[:n]
        excl = make_excl(ids, seed)
        cand = dev(ids.astype(np.int32))
        scores = dev(host)
        seg_ptr = dev(np.arange(rows + 1, dtype=np.int64) * n)
        for k in (7, 200):
            want_ids, want_vals = ops.topk_rows(scores, k, cand_ids=cand, excl=csr(excl))
            pos, vals, oid, status = ops.topk_segments(scores.reshape(-1), seg_ptr, k, ids=cand.repeat(rows), excl=csr(excl))
            torch.cuda.synchronize()
            assert torch.equal(oid, want_ids) and torch.equal(vals.view(torch.int32), want_vals.view(torch.int32))
            assert status.tolist() == [0, 0]
            p = pos.cpu().numpy()
            np.testing.assert_array_equal(np.where(p >= 0, ids[np.maximum(p, 0)], -1), want_ids.cpu().numpy())
        # named items: every third candidate of the row (some of them excluded), as ascending ids and as ascending positions
        col_of = {int(i): j for j, i in enumerate(ids)}
        named = [sorted(ids[r::3].tolist()) for r in range(rows)]
        pptr = np.zeros(rows + 1, np.int64)
        pptr[1:] = np.cumsum([len(x) for x in named])
        pids = np.concatenate(named).astype(np.int32)
        w_counts, w_vals, w_elig = (t.cpu().numpy() for t in ops.rank_positives(scores, (dev(pptr), dev(pids)), cand_ids=cand,
                                                                                excl=csr(excl)))
        q_rows = [sorted(col_of[i] for i in x) for x in named]
        q_pos = np.concatenate(q_rows).astype(np.int32)
        counts, vals, elig, status = (t.cpu().numpy() for t in ops.rank_segments(scores.reshape(-1), seg_ptr, (dev(pptr), dev(q_pos)),
                                                                                 ids=cand.repeat(rows), excl=csr(excl)))
        np.testing.assert_array_equal(elig, w_elig)
        assert status.tolist() == [0, 0]
        for r in range(rows):
            at = {p: pptr[r] + t for t, p in enumerate(q_rows[r])}
            for t, item in enumerate(named[r]):
                a, b = pptr[r] + t, at[col_of[item]]
                assert w_counts[a].tolist() == counts[b].tolist() and bits(w_vals[a:a + 1])[0] == bits(vals[b:b + 1])[0], (n, r, item)


@pytest.mark.parametrize("lengths,bound,form", [([5, 70, 3, 600, 64, 0], 64, None), ([5, 70, 3, 600, 64, 0], 64, "block"),
                                                ([700, 20, 650, 7000, 649], 650, None)])
def test_a_segment_over_the_bound_is_padding(hip_lib, lengths, bound, form):
    case = make_case(lengths, seed=21)
    over = [n > bound for n in lengths]
    k = 5
    got = run_topk(case, k, form=form, max_len=bound)
    want = want_topk(case, k, max_len=bound)
    same(got, want)
    assert got[3] == [sum(over), k * sum(over)]
    for s, o in enumerate(over):
        assert (got[0][s] == -1).all() == (o or lengths[s] == 0 or (case["ids"][case["ptr"][s]:case["ptr"][s + 1]] < 0).all())
    got = run_rank(case, form=form, max_len=bound)
    same(got, want_rank(case, max_len=bound))
    assert got[3][0] == sum(over) and (got[2] == -1).tolist() == over
    # the neighbours of the long segments are what they are without them
    keep = [s for s, o in enumerate(over) if not o]
    alone = run_topk(case, k, form=form)
    np.testing.assert_array_equal(got[2][keep], run_rank(case, form=form)[2][keep])
    np.testing.assert_array_equal(run_topk(case, k, form=form, max_len=bound)[0][keep], alone[0][keep])


# --------------------------------------------------------------------------- the feeder, end to end
def test_recommend_lists_of_one_candidate_array_equals_recommend(hip_lib):
    feeder = build_model(16, 4)
    rng = np.random.default_rng(5)
    users = rng.choice(40, 24, replace=False)
    items = np.sort(rng.choice(3000, 900, replace=False))
    rec = records(users, items, 6)
    k = 50
    want_items, want_scores = feeder.recommend(users, k, items, exclude=rec)
    got_items, got_scores, got_pos = feeder.recommend_lists(users, [items] * len(users), k, exclude=rec)
    torch.cuda.synchronize()
    assert got_items.dtype == torch.int64 and got_pos.dtype == torch.int32
    assert torch.equal(got_items, want_items) and torch.equal(got_scores.view(torch.int32), want_scores.view(torch.int32))
    np.testing.assert_array_equal(items[got_pos.cpu().numpy()], got_items.cpu().numpy())
    # the CSR form of the same lists, on the device
    ptr = torch.arange(len(users) + 1, dtype=torch.int64, device=DEV) * len(items)
    again = feeder.recommend_lists(users, (ptr, dev(np.tile(items, len(users)))), k, exclude=rec)
    assert all(torch.equal(a, b) for a, b in zip(again, (got_items, got_scores, got_pos)))


def test_feeder_ragged_lists_match_oracle(hip_lib):
    feeder = build_model(16, 4)
    rng = np.random.default_rng(9)
    users = rng.choice(40, 12, replace=False)
    lengths = [300, 1, 257, 0, 64, 65, 180, 299, 2, 170, 240, 222]
    lists = [rng.choice(3000, n, replace=False).astype(np.int64) for n in lengths]
    lists[4][::7] = -1                                                          # padded slots inside a list
    rec = {int(u): set(l[l >= 0][::5].tolist()) | {2999} for u, l in zip(users[::2], lists[::2])}
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum(lengths)
    flat_items = np.concatenate(lists)
    T = int(ptr[-1])
    max_pairs = 450                                                             # cuts lists across scoring pieces: pieces of 450, 450, 450, 450
    assert T == 1800 and T % max_pairs == 0
    u_exp = np.repeat(users, lengths)
    scores = np.concatenate([feeder.scores(u_exp[a:a + max_pairs], np.maximum(flat_items[a:a + max_pairs], 0)).cpu().numpy()
                             for a in range(0, T, max_pairs)])
    excl = [rec.get(int(u), set()) for u in users]
    ids32 = flat_items.astype(np.int32)
    k = 40
    w_pos, w_vals, w_ids, _ = topk_segments_oracle(scores, ptr, k, ids=ids32, excl=excl)
    items, vals, pos = feeder.recommend_lists(users, lists, k, exclude=rec, max_pairs=max_pairs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(pos.cpu().numpy(), w_pos)
    np.testing.assert_array_equal(items.cpu().numpy(), w_ids.astype(np.int64))
    np.testing.assert_array_equal(bits(vals.cpu().numpy()), w_vals)
    queries = [list(range(0, n + 1, 3)) for n in lengths]                       # the last of each may lie beyond the list
    q_ptr = np.zeros(len(lists) + 1, np.int64)
    q_ptr[1:] = np.cumsum([len(q) for q in queries])
    q_pos = np.concatenate([np.asarray(q, np.int32) for q in queries])
    w_counts, w_qv, w_elig, _ = rank_segments_oracle(scores, ptr, q_ptr, q_pos, ids=ids32, excl=excl)
    g_ptr, g_pos, counts, qv, elig = feeder.rank_lists(users, (ptr, flat_items), queries, exclude=rec, max_pairs=max_pairs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g_ptr.cpu().numpy(), q_ptr)
    np.testing.assert_array_equal(g_pos.cpu().numpy(), q_pos)
    np.testing.assert_array_equal(counts.cpu().numpy(), w_counts)
    np.testing.assert_array_equal(bits(qv.cpu().numpy()), w_qv)
    np.testing.assert_array_equal(elig.cpu().numpy(), w_elig)
    # whole-list chunks of another size, and one call for everything: the same results
    for mp in (450 * 2, 1 << 20):
        if T % mp in (0, T):
            same([t.cpu().numpy() for t in feeder.recommend_lists(users, lists, k, exclude=rec, max_pairs=mp)][2:], [w_pos])
