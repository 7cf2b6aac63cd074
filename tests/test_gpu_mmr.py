"""-m gpu: greedy MMR reranking inside per-user candidate lists.  mvin_mmr_segments against tests/mmr_oracle.py: bit for bit on
inputs where every product and sum is exact (all six outputs and status, both forms, every lane-group width, alone and among
300 other segments, under loose and tight bounds), against ops.topk_segments at lam = 1, a segment over the cap and broken
pointers, a table with NaN and inf rows, and on real-valued inputs step by step against float64 within a derived bound.
Output buffers are guarded as in test_gpu_segments.py."""
import numpy as np
import pytest
import torch

from mvin_amd import ops
from mmr_cases import REAL_SHAPES, exact_inputs, inv_norms64, real_case
from mmr_oracle import mmr_exact, mmr_follow, picks_valid
from test_gpu_segments import dev, guarded, guards_intact, make_case
from test_gpu_topk import bits, csr

pytestmark = pytest.mark.gpu

QNAN = 0x7FC00000
WAVE_LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 511, 512]
BLOCK_LENGTHS = [513, 1000, 4096, 9, 0]


def canon(x):
    """The bits of f32 values, every NaN as one pattern: 0 * inf is a NaN of either sign, depending on who multiplies."""
    x = np.asarray(x, np.float32)
    return np.where(np.isnan(x), np.uint32(QNAN), x.view(np.uint32))


def feat_of(inp):
    return dev(inp["buf"])[:, :inp["feat"].shape[1]]           # rows ld floats apart


def run_mmr(inp, k, lam, use_excl=True, feat=None, row_scale=None, **kw):
    """(pos, value bits, ids, mmr bits, pen bits, simsum bits, status) of one guarded call."""
    n_seg = len(inp["ptr"]) - 1
    outs = [guarded((n_seg, k), dt) for dt in (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32, torch.float32)]
    outs.append(guarded((2,), torch.int64))
    outs[6][0].zero_()
    if row_scale is None and inp.get("row_scale") is not None:
        row_scale = dev(inp["row_scale"])
    got = ops.mmr_segments(dev(inp["scores"]), dev(inp["ptr"]), dev(inp["ids"]), feat_of(inp) if feat is None else feat, k, lam,
                           row_scale=row_scale, excl=csr(inp["excl"]) if use_excl and inp.get("excl") is not None else None,
                           out=tuple(o for o, _ in outs), **kw)
    torch.cuda.synchronize()
    assert all(guards_intact(w) for _, w in outs), "a write outside an output buffer"
    pos, vals, oid, mmr, pen, simsum, status = (t.cpu().numpy() for t in got)
    return pos, bits(vals), oid, canon(mmr), canon(pen), canon(simsum), status.tolist()


def want_mmr(inp, k, lam, use_excl=True, max_len=None):
    pos, vals, oid, mmr, pen, simsum, status = mmr_exact(inp["scores"], inp["ptr"], inp["ids"], inp["feat"], k, lam,
                                                         row_scale=inp["row_scale"], excl=inp["excl"] if use_excl else None,
                                                         max_len=max_len)
    return pos, vals, oid, canon(mmr), canon(pen), canon(simsum), status


def prefix(want, k):
    return tuple(w[:, :k] for w in want[:6]) + (want[6],)


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=f"output {i}")


def eligible_count(inp, s):
    lo, hi = int(inp["ptr"][s]), int(inp["ptr"][s + 1])
    own = inp["ids"][lo:hi]
    return int(((own >= 0) & (own < inp["n_rows"]) & ~np.isin(own, np.fromiter(inp["excl"][s], np.int64, len(inp["excl"][s])))).sum())


# which, D, lam, scaled, ld: every D of the contract's corners and a row stride above D once; every lam of the exact cases
EXACT = [("wave", 4, 0.0, False, None), ("wave", 16, 0.25, True, None), ("wave", 64, 0.5, False, None), ("wave", 68, 1.0, True, 72),
         ("wave", 128, 0.5, True, None), ("wave", 256, 0.25, False, None),
         ("block", 16, 0.25, False, None), ("block", 64, 0.5, True, None), ("block", 256, 0.0, True, None)]


@pytest.mark.parametrize("which,D,lam,scaled,ld", EXACT)
def test_exact_inputs_match_the_oracle_bit_for_bit(hip_lib, which, D, lam, scaled, ld):
    cap = ops.segments_wave_cap()
    assert cap == 512 and ops.mmr_max_len() == 4096
    lengths = WAVE_LENGTHS if which == "wave" else BLOCK_LENGTHS
    inp = exact_inputs(make_case(lengths, seed=31 + D), D, seed=D, scaled=scaled, ld=ld)
    assert (inp["ids"] >= inp["n_rows"]).any() and (inp["ids"] < 0).any()      # ids beyond the table, and padding
    short = lengths.index(9)
    e9 = eligible_count(inp, short)
    ks = {1, 5, e9, e9 + 3, 64}
    if which == "wave":
        e65 = eligible_count(inp, lengths.index(65))
        ks |= {e65, e65 + 3}
    assert max(ks) <= 128                                                      # mmr_cases: the sums stay exact
    want = want_mmr(inp, max(ks), lam)
    assert want[0].min() == -1 and want[6] == [0, 0]
    for k in sorted(ks):
        ref = run_mmr(inp, k, lam)                                             # automatic: the form the case is named after
        same(ref, prefix(want, k))
        if which == "wave":
            same(run_mmr(inp, k, lam, form="wave"), ref)
        same(run_mmr(inp, k, lam, form="block"), ref)
    same(run_mmr(inp, 5, lam, use_excl=False), prefix(want_mmr(inp, 5, lam, use_excl=False), 5))
    with pytest.raises(Exception, match="form=1"):
        ops.mmr_segments(dev(inp["scores"]), dev(inp["ptr"]), dev(inp["ids"]), feat_of(inp), 5, lam, form="wave", max_len=cap + 1)


def test_k_1024_at_the_longest_segment(hip_lib):
    inp = exact_inputs(make_case([4096, 100], seed=41), 16, seed=42, scaled=False)
    want = want_mmr(inp, 1024, 0.5)
    got = run_mmr(inp, 1024, 0.5)
    same(got, want)
    assert (got[0][0] >= 0).all() and (got[0][1] == -1).any()                  # the long list fills every slot, the short one does not


@pytest.mark.parametrize("n", [65, 300, 600])
def test_a_segment_alone_among_300_others_and_under_a_tight_bound(hip_lib, n):
    """The same segment by itself, between 300 short ones, and under bounds that pick another lane-group width or form."""
    rng = np.random.default_rng(n)
    others = rng.integers(0, 41, 300).tolist()
    lengths = others[:150] + [n] + others[150:]
    D, lam, k = 64, 0.5, 20
    whole = exact_inputs(make_case(lengths, seed=50 + n), D, seed=51 + n, scaled=True)
    s = 150
    lo, hi = int(whole["ptr"][s]), int(whole["ptr"][s + 1])
    alone = dict(whole, ptr=np.asarray([0, n], np.int64), scores=whole["scores"][lo:hi], ids=whole["ids"][lo:hi], excl=[whole["excl"][s]])
    want = want_mmr(alone, k, lam)
    same(run_mmr(alone, k, lam), want)
    for bound in (n, 512, 513, 4096):
        if bound >= n:
            same(run_mmr(alone, k, lam, max_len=bound), want)
    got = run_mmr(whole, k, lam)
    same([g[s:s + 1] for g in got[:6]], want[:6])
    same(got, want_mmr(whole, k, lam))


@pytest.mark.parametrize("which", ["wave", "block"])
def test_lam_one_is_topk_segments(hip_lib, which):
    lengths = WAVE_LENGTHS if which == "wave" else [513, 1000, 9, 2000]
    inp = exact_inputs(make_case(lengths, seed=61), 16, seed=62, scaled=True, all_rows=True)
    scores, ptr, ids, feat, excl = dev(inp["scores"]), dev(inp["ptr"]), dev(inp["ids"]), feat_of(inp), csr(inp["excl"])
    for k in (5, 64):
        pos, vals, oid, status = ops.topk_segments(scores, ptr, k, ids=ids, excl=excl)
        got = ops.mmr_segments(scores, ptr, ids, feat, k, 1.0, row_scale=dev(inp["row_scale"]), excl=excl)
        torch.cuda.synchronize()
        assert torch.equal(got[0], pos) and torch.equal(got[1].view(torch.int32), vals.view(torch.int32)) and torch.equal(got[2], oid)
        assert got[6].tolist() == status.tolist() == [0, 0]


@pytest.mark.parametrize("lengths,bound,form", [([5, 4097, 70], 4096, None), ([5, 70, 3, 600, 64, 0], 64, None),
                                                ([5, 70, 3, 600, 64, 0], 64, "block")])
def test_a_segment_over_the_bound_is_padding(hip_lib, lengths, bound, form):
    k = 5
    inp = exact_inputs(make_case(lengths, seed=71), 16, seed=72, scaled=False)
    over = [n > bound for n in lengths]
    got = run_mmr(inp, k, 0.5, max_len=bound, form=form)
    same(got, want_mmr(inp, k, 0.5, max_len=bound))
    assert got[6] == [sum(over), k * sum(over)]
    for s, o in enumerate(over):
        if o:
            assert (got[0][s] == -1).all() and (got[2][s] == -1).all() and (got[1][s] == 0xFF800000).all()
            assert not got[3][s].any() and not got[4][s].any() and not got[5][s].any()
    if max(lengths) > ops.mmr_max_len():
        with pytest.raises(ValueError, match="4096"):                          # the bound read from seg_ptr is over the cap
            ops.mmr_segments(dev(inp["scores"]), dev(inp["ptr"]), dev(inp["ids"]), feat_of(inp), k, 0.5)


@pytest.mark.parametrize("form", [None, "block"])
def test_broken_pointers_are_padding(hip_lib, form):
    k = 6
    inp = exact_inputs(make_case([100], seed=81), 16, seed=82, scaled=False)
    inp = dict(inp, ptr=np.asarray([0, 50, 30, 100, 120], np.int64), excl=[set(), set(), set(), set()])   # backwards, then past the end
    got = run_mmr(inp, k, 0.25, max_len=100, form=form)
    assert got[6] == [2, 2 * k]
    for s in (1, 3):
        assert (got[0][s] == -1).all() and (got[2][s] == -1).all()
    for s, (lo, hi) in ((0, (0, 50)), (2, (30, 100))):                          # the sound segments are what they are by themselves
        one = dict(inp, ptr=np.asarray([0, hi - lo], np.int64), scores=inp["scores"][lo:hi], ids=inp["ids"][lo:hi], excl=[set()])
        same([g[s:s + 1] for g in got[:6]], want_mmr(one, k, 0.25)[:6])


@pytest.mark.parametrize("which", ["wave", "block"])
def test_nan_and_inf_rows_leave_distinct_eligible_picks(hip_lib, which):
    lengths = [0, 1, 9, 65, 300, 512] if which == "wave" else [513, 1500, 9]
    inp = exact_inputs(make_case(lengths, seed=91), 16, seed=92, scaled=True)
    rng = np.random.default_rng(93)
    bad = rng.choice(inp["n_rows"], inp["n_rows"] // 6, replace=False)
    inp["buf"][bad[0::3], :] = np.nan
    inp["buf"][bad[1::3], 3] = np.inf
    inp["buf"][bad[2::3], 5] = -np.inf
    for k in (7, 64):
        got = run_mmr(inp, k, 0.5)                                             # the guards are checked inside
        assert got[6] == [0, 0]
        for s in range(len(lengths)):
            lo, hi = int(inp["ptr"][s]), int(inp["ptr"][s + 1])
            assert picks_valid(inp["ids"][lo:hi], inp["n_rows"], inp["excl"][s], got[0][s]), (which, k, s)
            p = got[0][s][got[0][s] >= 0]
            np.testing.assert_array_equal(got[2][s][:len(p)], inp["ids"][lo:hi][p])
            np.testing.assert_array_equal(got[1][s][:len(p)], bits(inp["scores"][lo:hi][p]))


def test_row_inv_norms_against_float64(hip_lib):
    rng = np.random.default_rng(7)
    for n_rows, D, ld in ((1, 4, 4), (33, 16, 16), (257, 68, 72), (1000, 256, 256)):
        buf = (rng.normal(0.0, 1.0, (n_rows, ld)) * np.exp(rng.normal(0.0, 4.0, (n_rows, 1)))).astype(np.float32)
        buf[0, :] = 0.0                                                        # a zero row: 1 / eps
        got = ops.row_inv_norms(dev(buf)[:, :D]).cpu().numpy()
        want = inv_norms64(buf[:, :D])
        assert got[0] == np.float32(1e12)
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 * np.spacing(want.astype(np.float32)).astype(np.float64)).all()


@pytest.mark.parametrize("n,D,k,lam", REAL_SHAPES)
def test_real_valued_picks_follow_float64(hip_lib, n, D, k, lam):
    """A greedy rule has no tolerance of its own, so float64 follows the kernel's picks: at every step the picked entry's
    float64 value is within the derived bound of the best one, and the three f32 outputs are within theirs."""
    case = real_case(n, D, seed=1000 + n)
    feat = dev(case["feat"])
    rs = ops.row_inv_norms(feat)
    rs_host = rs.cpu().numpy()
    want_rs = inv_norms64(case["feat"])
    assert (np.abs(rs_host.astype(np.float64) - want_rs) <= 2.0 * np.spacing(want_rs.astype(np.float32)).astype(np.float64)).all()
    inp = dict(case, excl=None, buf=case["feat"])
    forms = [None] + (["block"] if n <= ops.segments_wave_cap() else [])
    for form in forms:
        got = run_mmr(inp, k, lam, feat=feat, row_scale=rs, form=form)
        same(run_mmr(inp, k, lam, feat=feat, row_scale=rs, form=form), got)    # two launches, the same bits
        assert got[6] == [0, 0]
        mmr, pen, simsum = (g.view(np.float32).astype(np.float64) for g in got[3:6])
        for s in range(len(case["ptr"]) - 1):
            lo, hi = int(case["ptr"][s]), int(case["ptr"][s + 1])
            f = mmr_follow(case["scores"][lo:hi], case["ids"][lo:hi], case["feat"], lam, got[0][s], row_scale=rs_host)
            assert f["valid"] and len(f["value"]) == k
            print(f"n={n} D={D} form={form} list {s}: worst shortfall {np.max(f['best'] - f['value']):.3e} "
                  f"(bound {np.min(f['tol_pick'] + f['tol_best']):.3e} .. {np.max(f['tol_pick'] + f['tol_best']):.3e}), "
                  f"|mmr| {np.max(np.abs(mmr[s] - f['value'])):.3e} |pen| {np.max(np.abs(pen[s] - f['pen'])):.3e} "
                  f"|simsum| {np.max(np.abs(simsum[s] - f['simsum'])):.3e} (bound {np.max(f['tol_simsum']):.3e})")
            assert (f["value"] >= f["best"] - (f["tol_pick"] + f["tol_best"])).all(), (form, s)
            assert (np.abs(mmr[s] - f["value"]) <= f["tol_pick"]).all(), (form, s)
            assert (np.abs(pen[s] - f["pen"]) <= f["tol_pen"]).all(), (form, s)
            assert (np.abs(simsum[s] - f["simsum"]) <= f["tol_simsum"]).all(), (form, s)
