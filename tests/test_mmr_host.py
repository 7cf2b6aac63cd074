"""CPU: the MMR rule by hand and against the top-K oracle, the new entry points' refusals (codes, nothing launched), the
ValueErrors of ops.mmr_segments / DeviceFeeder.diversify_lists / harness.diversity_eval, diversity_eval's numbers on a stubbed
feeder, and the non-vacuity of the real-valued GPU cases (tests/test_gpu_mmr.py) shown on the oracle alone."""
import ctypes as C
import types

import numpy as np
import pytest

from mmr_cases import REAL_SHAPES, real_case
from mmr_oracle import images, mmr_exact, mmr_follow, mmr_greedy64, picks_valid
from segments_oracle import score_image, topk_segments_oracle


def canon(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))


def test_vectorised_image_is_score_image():
    vals = np.float32([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38, 0.125])
    vals = np.concatenate([vals, np.random.default_rng(0).standard_normal(200).astype(np.float32)])
    assert images(vals).tolist() == [score_image(v) for v in vals]
    assert images(np.float32([-np.nan]))[0] == 0


def test_the_rule_by_hand():
    """Six entries, lam = 1/2.  Step 0 takes the best score; step 1 would take entry 1 by score, but it repeats entry 0's row
    (penalty 4), so entries 2 and 4 tie at 0.75 and the lower position wins; entry 4 then carries entry 2's penalty."""
    feat = np.float32([[2, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0], [0, 2, 0, 0], [0, 0, 0, 1]])
    scores = np.float32([2.0, 1.75, 1.5, 0.5, 1.5, 0.25])
    ids = np.arange(6, dtype=np.int32)
    pos, vals, oid, mmr, pen, simsum, status = mmr_exact(scores, [0, 6], ids, feat, 8, 0.5)
    assert pos[0].tolist() == [0, 2, 3, 5, 1, 4, -1, -1] and oid[0].tolist() == [0, 2, 3, 5, 1, 4, -1, -1]
    assert mmr[0].tolist() == [1.0, 0.75, 0.25, 0.125, -1.125, -1.25, 0.0, 0.0]
    assert pen[0].tolist() == [0.0, 0.0, 0.0, 0.0, 4.0, 4.0, 0.0, 0.0]
    assert simsum[0].tolist() == [0.0, 0.0, 0.0, 0.0, 4.0, 4.0, 0.0, 0.0]
    assert vals[0].tolist() == scores[[0, 2, 3, 5, 1, 4]].view(np.uint32).tolist() + [0xFF800000] * 2 and status == [0, 0]
    assert topk_segments_oracle(scores, [0, 6], 8)[0][0].tolist() == [0, 1, 2, 4, 3, 5, -1, -1]      # what the penalty changed
    # a row scale of 1/2 on entries 0 and 1 makes their similarity 1: entry 1 (0.875 - 0.5) still loses step 1 but wins step 2
    rs = np.float32([0.5, 0.5, 1, 1, 1, 1])
    pos, _, _, mmr, pen, simsum, _ = mmr_exact(scores, [0, 6], ids, feat, 3, 0.5, row_scale=rs)
    assert pos[0].tolist() == [0, 2, 1] and mmr[0].tolist() == [1.0, 0.75, 0.375] and pen[0].tolist() == [0.0, 0.0, 1.0]
    assert simsum[0].tolist() == [0.0, 0.0, 1.0]
    # the float64 walk agrees with itself and with the f32 rule on these exact numbers
    g = mmr_greedy64(scores, ids, feat, 0.5, 8)
    assert g["picks"] == [0, 2, 3, 5, 1, 4, -1, -1] and g["margin"][1] == 0.0 and g["value"].tolist() == [1.0, 0.75, 0.25, 0.125, -1.125, -1.25]
    f = mmr_follow(scores, ids, feat, 0.5, [0, 4, 3, 5, 1, 2, -1, -1])           # the other side of the tie: still within bounds
    assert f["valid"] and (f["value"] >= f["best"] - (f["tol_pick"] + f["tol_best"])).all()
    assert not mmr_follow(scores, ids, feat, 0.5, [0, 0, 3])["valid"] and not mmr_follow(scores, ids, feat, 0.5, [0, -1, -1])["valid"]
    assert picks_valid(ids, 6, {2}, [0, 1, 3, 4, 5, -1]) and not picks_valid(ids, 6, {2}, [0, 2, 3, 4, 5, -1])
    assert not picks_valid(ids, 4, None, [0, 1, 2, 3, 4])                        # entry 4 has no row in a table of 4


def small_case(seed):
    rng = np.random.default_rng(seed)
    lengths = [0, 1, 7, 20, 33]
    ptr = np.zeros(len(lengths) + 1, np.int64)
    ptr[1:] = np.cumsum(lengths)
    T = int(ptr[-1])
    scores = (rng.integers(-16, 17, T) / 8.0).astype(np.float32)
    scores[rng.choice(T, 8, replace=False)] = np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, np.inf, -0.0])
    ids = rng.integers(0, 40, T).astype(np.int32)
    ids[rng.random(T) < 0.11] = -1
    excl = [set(), set(), {int(ids[ptr[2]])} if ids[ptr[2]] >= 0 else set(), set(ids[ptr[3]:ptr[3] + 3].tolist()), set()]
    feat = rng.integers(-3, 4, (40, 8)).astype(np.float32)
    return ptr, scores, ids, excl, feat


def test_lam_one_is_the_topk_oracle_and_lam_zero_starts_in_position_order():
    ptr, scores, ids, excl, feat = small_case(3)
    for k in (1, 5, 40):
        pos, vals, oid, mmr, pen, simsum, status = mmr_exact(scores, ptr, ids, feat, k, 1.0, excl=excl)
        w_pos, w_vals, w_ids, w_status = topk_segments_oracle(scores, ptr, k, ids=ids, excl=excl)
        assert pos.tolist() == w_pos.tolist() and vals.tolist() == w_vals.tolist() and oid.tolist() == w_ids.tolist() and status == w_status
    finite = np.where(np.isfinite(scores), scores, np.float32(0.5))
    pos = mmr_exact(finite, ptr, ids, feat, 3, 0.0, excl=excl)[0]
    for s in range(len(ptr) - 1):
        own = ids[ptr[s]:ptr[s + 1]]
        el = [p for p in range(len(own)) if own[p] >= 0 and int(own[p]) not in excl[s]]
        assert pos[s, 0] == (el[0] if el else -1)
    # an id beyond the table is not eligible; a segment over the bound is padding and counted
    pos = mmr_exact(scores, ptr, ids, feat[:20], 40, 0.5)[0]
    assert all(ids[ptr[s] + p] < 20 for s in range(len(ptr) - 1) for p in pos[s] if p >= 0)
    *_, status = mmr_exact(scores, ptr, ids, feat, 4, 0.5, max_len=20)
    assert status == [1, 4]


def test_the_new_symbols_exist(hip_lib):
    from mvin_amd import _lib, harness, ops
    for name in ("mvin_mmr_max_len", "mvin_row_inv_norms", "mvin_mmr_segments"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES
    assert hip_lib.mvin_mmr_max_len() == ops.mmr_max_len() == 4096 and hip_lib.mvin_abi_version() == 12
    assert callable(ops.mmr_segments) and callable(ops.row_inv_norms)
    assert callable(harness.DeviceFeeder.diversify_lists) and callable(harness.diversity_eval)


def test_entry_points_refuse_on_the_host(hip_lib):
    """Every refusal of the contract comes back as its code with nothing but fake pointers given: nothing is launched."""
    one = C.c_void_p(16)

    def mmr(**kw):
        a = dict(scores=one, total=10, seg_ptr=one, n_seg=2, ids=one, excl_ptr=None, excl_ids=None, feat=one, n_rows=5, D=8, ld=8,
                 row_scale=None, lam=0.5, k=3, max_len=8, form=0, out_pos=one, out_vals=one, out_ids=one, out_mmr=None, out_pen=None,
                 out_simsum=None, status=one, stream=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return hip_lib.mvin_mmr_segments(*a.values())

    err = hip_lib.mvin_last_error
    assert mmr(n_seg=0) == 0                                                   # accepted, and launches nothing
    for bad in (dict(k=0), dict(k=1025), dict(lam=-0.125), dict(lam=1.5), dict(lam=float("nan")), dict(lam=float("inf")),
                dict(max_len=4097), dict(max_len=-1), dict(form=3), dict(form=-1), dict(form=1, max_len=513), dict(D=2), dict(D=260),
                dict(D=6, ld=8), dict(ld=4), dict(ld=10), dict(n_rows=-1), dict(n_rows=1 << 31), dict(n_seg=-1), dict(total=-1),
                dict(feat=C.c_void_p(20))):
        assert mmr(**bad) == -2, bad
    assert mmr(form=1, max_len=513) == -2 and b"form=1" in err()
    assert mmr(lam=1.5) == -2 and b"lam" in err()
    for bad in (dict(scores=None), dict(seg_ptr=None), dict(ids=None), dict(feat=None), dict(out_pos=None), dict(out_vals=None),
                dict(out_ids=None), dict(status=None), dict(excl_ptr=one), dict(excl_ids=one)):
        assert mmr(**bad) == -1, bad
    assert mmr(n_seg=0, excl_ptr=one, excl_ids=one, row_scale=one, out_mmr=one, out_pen=one, out_simsum=one, form=2, max_len=4096,
               D=256, ld=260, k=1024, lam=1.0) == 0
    assert mmr(n_seg=0, form=1, max_len=512, lam=0.0, D=4, ld=4, n_rows=0, feat=None) == 0

    norms = hip_lib.mvin_row_inv_norms
    assert norms(one, 0, 8, 8, 1e-12, one, None) == 0                          # no rows: nothing launched
    for D, ld in ((2, 4), (260, 260), (6, 8), (8, 4), (8, 10)):
        assert norms(one, 0, D, ld, 1e-12, one, None) == -2
    assert norms(one, -1, 8, 8, 1e-12, one, None) == -2
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert norms(one, 0, 8, 8, eps, one, None) == -2 and b"eps" in err()
    assert norms(None, 3, 8, 8, 1e-12, one, None) == -1 and norms(one, 3, 8, 8, 1e-12, None, None) == -1


def stub_feeder(table):
    from mvin_amd import harness
    feeder = harness.DeviceFeeder.__new__(harness.DeviceFeeder)
    feeder.model = types.SimpleNamespace(device="cpu", entity_emb_matrix=table)
    return feeder


def test_python_layers_refuse_bad_arguments(hip_lib):
    import torch
    from mvin_amd import harness, ops
    scores, ptr, ids = torch.zeros(4), torch.tensor([0, 4]), torch.zeros(4, dtype=torch.int32)
    feat = torch.zeros(6, 8)
    for kw in (dict(k=0), dict(k=1025), dict(lam=-0.1), dict(lam=1.01), dict(lam=float("nan")), dict(ids=None),
               dict(feat=feat.to(torch.bfloat16)), dict(feat=torch.zeros(6, 6)), dict(feat=torch.zeros(6, 260)), dict(feat=torch.zeros(8))):
        a = dict(scores=scores, seg_ptr=ptr, ids=ids, feat=feat, k=2, lam=0.5)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.mmr_segments(**a)
    with pytest.raises(ValueError, match="bf16"):
        ops.row_inv_norms(feat.to(torch.bfloat16))
    with pytest.raises(ValueError, match="eps"):
        ops.row_inv_norms(feat, eps=0.0)
    # the feeder: a bf16 table, a table that is no table, a list over the cap (named by its user), a bad max_pairs
    with pytest.raises(ValueError, match="bf16"):
        stub_feeder(feat.to(torch.bfloat16)).diversify_lists([3], [[1, 2]], 2)
    with pytest.raises(ValueError, match="bf16"):
        stub_feeder(feat).diversify_lists([3], [[1, 2]], 2, features=feat.to(torch.bfloat16))
    with pytest.raises(ValueError, match="max_pairs"):
        stub_feeder(feat).diversify_lists([3], [[1, 2]], 2, max_pairs=0)
    with pytest.raises(ValueError, match="user 11 .* 4097 entries"):
        stub_feeder(feat).diversify_lists([3, 11], [[1, 2], np.zeros(ops.mmr_max_len() + 1, np.int64)], 2)
    # diversity_eval
    for kw in (dict(k=0), dict(lams=()), dict(lams=(0.5, 1.5)), dict(truth_record=[1, 2]), dict(n_item=0)):
        a = dict(feeder=stub_feeder(feat), users=[3], lists=[[1, 2]], truth_record={3: {1}}, k=2)
        a.update(kw)
        with pytest.raises(ValueError, match="diversity_eval"):
            harness.diversity_eval(**a)


def test_diversity_eval_numbers_on_a_stubbed_feeder():
    """Two users, k = 3, returns fixed per lam: the row of lam = 1.0 and of lam = 0.5 by hand."""
    import torch
    from mvin_amd import harness
    fixed = {1.0: ([[5, 6, 7], [8, 9, -1]], [[0, .5, .75], [0, .25, 0]], [[0, .5, 1.0], [0, .25, 0]]),
             0.5: ([[5, 7, 2], [9, 8, -1]], [[0, .25, .25], [0, .25, 0]], [[0, .25, .5], [0, .25, 0]])}
    calls = []

    class Stub:
        model = types.SimpleNamespace(entity_emb_matrix=np.zeros((50, 4), np.float32))

        def diversify_lists(self, users, lists, k, lam=0.5, **kw):
            calls.append((lam, k, sorted(kw)))
            items, pen, simsum = fixed[lam]
            return (torch.tensor(items, dtype=torch.int64), torch.zeros(2, k), torch.zeros(2, k, dtype=torch.int32),
                    torch.tensor(pen, dtype=torch.float32), torch.tensor(simsum, dtype=torch.float32))

    rows = harness.diversity_eval(Stub(), [4, 1], None, {4: {6, 2, 30}, 1: set(), 9: {8}}, 3, lams=(1.0, 0.5), n_item=20)
    assert [c[:2] for c in calls] == [(1.0, 3), (0.5, 3)] and [r["lam"] for r in rows] == [1.0, 0.5]
    a, b = rows
    assert a["items"].tolist() == fixed[1.0][0] and a["items"].dtype == np.int64
    assert a["n_users"] == 1 and a["n_lists"] == 2                             # user 1 has no truth; both lists hold two picks
    assert a["recall"] == 1 / 3 and a["ndcg"] == (1 / np.log2(3)) / 1.0
    assert a["ild"] == np.mean([1 - 1.5 / 3, 1 - 0.25 / 1]) and a["coverage"] == 5 / 20 and a["penalty"] == np.mean([.5, .75, .25])
    assert b["recall"] == 1 / 3 and b["ndcg"] == (1 / np.log2(4)) / 1.0         # item 2 in slot 2
    assert b["ild"] == np.mean([1 - 0.75 / 3, 1 - 0.25 / 1]) and b["coverage"] == 5 / 20 and b["penalty"] == np.mean([.25, .25, .25])
    rows = harness.diversity_eval(Stub(), [4, 1], None, {}, 3, lams=[1.0])      # nobody has truth; the table's rows are the catalogue
    assert rows[0]["recall"] == 0.0 and rows[0]["n_users"] == 0 and rows[0]["coverage"] == 5 / 50


@pytest.mark.parametrize("n,D,k,lam", REAL_SHAPES)
def test_real_valued_cases_are_not_vacuous(n, D, k, lam):
    """On the inputs tests/test_gpu_mmr.py follows in float64: near-ties are rare (at most 5 % of the steps have a runner-up
    within the tolerance, so the bound decides little) and the penalty matters (every list differs from plain top-K)."""
    case = real_case(n, D, seed=1000 + n)
    near = steps = 0
    for s in range(len(case["ptr"]) - 1):
        lo, hi = int(case["ptr"][s]), int(case["ptr"][s + 1])
        sc, ids = case["scores"][lo:hi], case["ids"][lo:hi]
        g = mmr_greedy64(sc, ids, case["feat"], lam, k, row_scale=case["row_scale"])
        assert g["valid"] and min(g["picks"]) >= 0 and n >= 2 * k
        tol = g["tol_pick"] + g["tol_best"]
        assert 0.0 < tol[1:].max() < 1e-4                                      # about 1e-5 at these magnitudes
        near += int((g["margin"] <= tol).sum())
        steps += k
        assert lam <= 0.7 and g["picks"] != np.argsort(-sc.astype(np.float64), kind="stable")[:k].tolist(), s
    assert near <= 0.05 * steps, (near, steps)
