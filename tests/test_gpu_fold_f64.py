"""The folded score forms against float64, at the small shapes where their batching can go wrong.

mvin_fold_tables -> mvin_score_l2_folded_fwd (dim 64: mvin_fused_agg.hip, dim 32: mvin_fused_agg32.hip) and mvin_fold_tables_ex(aggregates = 0) ->
mvin_score_l2_folded_gather_fwd (mvin_fused_wpp_fold.hip) against tests/fold_ref.py -- the UNFOLDED formulas of include/mvin_hip.h on the plain
adjacency, which shares neither a projected table nor the encoded adjacency with them.  Batches of 16 pairs, quads of 4 (octets of 8 at dim 32)
and tiles of 32 each full, one short and one over; both softmax forms, one-sided (the entry points take t0 and t1 independently) and no
attention; with / without biases; both id widths; runs of one item; ids out of range (int64 ids with a high word set among them: the folded
entry points read the low 32-bit word; the two-launch variant of dim 64 is held to the same in test_gpu_fold_two_launch.py); user_o being q itself; want_item_emb = False; one
relation and the LDS limit of 2 600; tables below and just above one 16-row tile of the table builders.  Every launch runs twice and must give
the same bits.

Tolerance.  Per case and output, err_hip = max |kernel - float64| must stay within 4 x err_f32 + 2e-6, err_f32 = max |fp32 evaluation of the
SAME reference - float64| (the rule of test_random_configuration_in_folded_form; the yardstick never is the code under test).  err_f32 is
taken over at least YARDSTICK_PAIRS = 256 pairs drawn like the case's own, which are the first B of them: the maximum of a handful of draws
is no yardstick -- with these weights (normal x 0.3 at dim 64: |item_emb| up to 45, |scores| up to 55, one ulp = 3.8e-6) the fp32 reference
of a batch of ONE pair landed 1.7e-7 from float64 by chance while every correctly rounded fp32 evaluation may be 2e-6 and more away; over
the case's own pairs the rule missed in batches of 1 .. 17 pairs by up to 1.8 x while over all cases err_hip was 0.8 .. 1.2 x err_f32.
On top of it the tail kernel's absolute bounds against float64 (test_gpu_tail.py: item embeddings rtol 1e-5 / atol 2e-6, scores 1e-5 / 4e-6,
sigmoid 1e-5 / 1e-6) are asserted for the (form, output) pairs of TAIL_BOUNDS_HOLD -- those that meet them in every case of this module.
The others miss them at these magnitudes exactly as the fp32 reference does (its err_f32 is as large as err_hip) and keep the relative rule.

MEASURED on an MI355X, worst over all cases of this module (err_hip | err_f32 | err_hip / (4 err_f32 + 2e-6) | error / absolute bound):
    fold-D64K16    item_emb 2.9e-5 | 3.2e-5 | 0.32 | 5.04    scores 3.6e-5 | 4.3e-5 | 0.28 | 3.93    sigmoid 4.3e-6 | 6.3e-6 | 0.44 | 0.89
    fold-D64K32    item_emb 2.7e-5 | 3.8e-5 | 0.29 | 5.92    scores 5.0e-5 | 5.2e-5 | 0.38 | 2.84    sigmoid 4.0e-6 | 6.1e-6 | 0.31 | 1.04
    fold-D64K64    item_emb 3.3e-5 | 2.8e-5 | 0.31 | 6.45    scores 3.7e-5 | 4.7e-5 | 0.44 | 3.86    sigmoid 6.3e-6 | 7.2e-6 | 0.56 | 1.29
    fold-D32K16    item_emb 5.1e-6 | 7.0e-6 | 0.25 | 1.03    scores 6.0e-6 | 1.1e-5 | 0.26 | 0.51    sigmoid 6.9e-7 | 1.7e-6 | 0.17 | 0.19
    fold-D32K32    item_emb 5.5e-6 | 6.5e-6 | 0.34 | 1.25    scores 6.8e-6 | 9.0e-6 | 0.35 | 0.56    sigmoid 1.0e-6 | 1.2e-6 | 0.21 | 0.23
    gather-D64K16  item_emb 2.9e-5 | 3.2e-5 | 0.32 | 5.04    scores 3.6e-5 | 4.3e-5 | 0.30 | 3.28    sigmoid 3.6e-6 | 6.3e-6 | 0.37 | 0.69
    gather-D64K32  item_emb 2.7e-5 | 3.8e-5 | 0.29 | 5.15    scores 4.4e-5 | 5.2e-5 | 0.42 | 3.30    sigmoid 3.9e-6 | 6.1e-6 | 0.29 | 0.91
The per-row tables (TA1 | TA2 | T0A | M0, and H0 | G) met rtol 2e-5 / atol 5e-6 against their float64 definitions everywhere.  Run with -s for
the figures of a run (lines starting with MEASURED).
"""
import functools
import types

import numpy as np
import pytest
import torch

from fold_ref import clamp_ids, compare, fold_reference, fold_tables_reference, report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORMS = [("fold", 64, 16), ("fold", 64, 32), ("fold", 64, 64), ("fold", 32, 16), ("fold", 32, 32), ("gather", 64, 16), ("gather", 64, 32)]
FORM_IDS = ["%s-D%dK%d" % f for f in FORMS]
ATTENTION = ["unit", "sharp", "none", "t0", "t1"]            # logits at scale 1 / at scale 130 (per-row-maximum softmax) / absent / one-sided
PATTERNS = ["stride", "same", "runs", "oob"]
N_ENTITY = 603
# (form, output) pairs that meet the tail kernel's absolute bounds against float64 in every case of this module (the others keep the relative rule)
TAIL_BOUNDS_HOLD = {("fold-D32K16", "scores"), ("fold-D32K16", "sigmoid"), ("fold-D32K32", "scores"), ("fold-D32K32", "sigmoid"),
                    ("fold-D64K16", "sigmoid"), ("gather-D64K16", "sigmoid"), ("gather-D64K32", "sigmoid")}
YARDSTICK_PAIRS = 256
STATS = {}


def batch_sizes(K):
    return [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 4 * K + 37]


def pattern_cases(K):
    """(B, attention, int64 ids, user_o is q, biases) of test_item_patterns_against_float64, per pattern."""
    return ((4 * K + 37, "unit", True, False, True), (4 * K + 37, "none", False, True, False), (33, "sharp", False, False, True),
            (17, "t1", True, True, True))


def small_table_cases(K):
    """(B, attention, relations, int64 ids, biases) of test_tables_around_one_tile_of_rows, per table size."""
    return ((1, "unit", 7, True, True), (5, "none", 1, False, False), (17, "unit", 1, False, True), (33, "t0", 7, True, False),
            (4 * K + 37, "unit", 7, True, True))


@functools.lru_cache(maxsize=None)
def _world(D, K, n_entity, nR, kind, dev=DEV):
    """Tables, adjacency and parameters of one shape, built once and left unchanged.  kind "counts": nd = x % K + 1 distinct slots in row x, so
    every distinct-children count occurs as parent and as child; "random": uniform slots (tables smaller than K rows)."""
    rng = np.random.default_rng([D, K, n_entity, nR, len(kind)])
    if kind == "counts":
        adj_e = np.zeros((n_entity, K), dtype=np.int64)
        adj_r = np.zeros((n_entity, K), dtype=np.int64)
        for x in range(n_entity):
            nd = x % K + 1
            ne = rng.choice(n_entity, nd, replace=False)
            nr = rng.integers(0, nR, nd)
            pick = np.concatenate([np.arange(nd), rng.integers(0, nd, K - nd)])
            rng.shuffle(pick)
            adj_e[x], adj_r[x] = ne[pick], nr[pick]
    else:
        adj_e = rng.integers(0, n_entity, (n_entity, K))
        adj_r = rng.integers(0, nR, (n_entity, K))
    f = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32) * 0.3).to(dev)      # noqa: E731
    w = types.SimpleNamespace(D=D, K=K, n_entity=n_entity, nR=nR, kind=kind)
    w.E = f(n_entity, D)
    w.ae, w.ar = torch.from_numpy(adj_e.astype(np.int32)).to(dev), torch.from_numpy(adj_r.astype(np.int32)).to(dev)
    w.W0, w.W1, w.W2, w.A0, w.A1, w.Wmix = f(D, D), f(D, D), f(D, D), f(D, D), f(D, D), f(3 * D, D)
    w.bias = tuple(f(D) for _ in range(6))                    # b0, b1, b2, a0, a1, bmix
    w.unit = (f(nR), f(nR))
    def sharp():                                              # scale 130; seven draws do not always spread past the kernels' threshold of 60
        while True:
            t = f(nR) * 130.0
            if nR == 1 or float(t.max() - t.min()) > 60:
                return t
    w.sharp = (sharp(), sharp())
    w.enc = None
    return w


def _enc(w):
    from mvin_amd import ops
    if w.enc is None:
        w.enc = ops.encode_adjacency(w.ae, w.ar)
        if w.kind == "counts":
            assert sorted(set(w.enc[2].cpu().tolist())) == list(range(1, w.K + 1))
    return w.enc


def _logits(w, att):
    t0, t1 = w.sharp if att == "sharp" else w.unit
    if att == "sharp":
        assert float(t0.max() - t0.min()) > 60 and float(t1.max() - t1.min()) > 60
    return (t0 if att in ("unit", "sharp", "t0") else None), (t1 if att in ("unit", "sharp", "t1") else None)


def _items(pattern, B, n_entity, i64, seed=0):
    i = np.arange(B)
    if pattern in ("stride", "oob"):
        x = i * 7 % n_entity
    elif pattern == "same":
        x = np.full(B, (5 + seed) % n_entity)
    else:                                                     # sorted runs: item j of the walk repeats j % 9 + 1 times
        ids = np.sort((np.arange(B) * 3 + seed) % n_entity)
        x = np.repeat(ids, np.arange(B) % 9 + 1)[:B]
    x = x.astype(np.int64)
    if pattern == "oob":
        x[::7] = n_entity + 12345
        if not i64:
            x[::14] = -1
    return torch.from_numpy(x.astype(np.int64 if i64 else np.int32)).to(DEV)


def _case(w, pattern, B, i64, uo_is_q, seed, item_seed=0):
    """The case's B pairs (items, q, user_o) as the first rows of at least YARDSTICK_PAIRS pairs drawn the same way: the fp32 yardstick is
    taken over all of them (see the module's docstring), the kernels get the first B."""
    n = max(B, YARDSTICK_PAIRS)
    g = torch.Generator(device="cpu").manual_seed(seed)
    ext_items = _items(pattern, n, w.n_entity, i64, item_seed)
    ext_q = (torch.randn(n, w.D, generator=g) * 0.3).to(DEV)
    ext_uo = ext_q if uo_is_q else (torch.randn(n, w.D, generator=g) * 0.3).to(DEV)
    q = ext_q[:B]
    return types.SimpleNamespace(B=B, items=ext_items[:B], q=q, uo=q if uo_is_q else ext_uo[:B], ext=(ext_items, ext_q, ext_uo))


def _tables(w, form, t0, bias):
    from mvin_amd import ops
    enc_e, enc_r, _ = _enc(w)
    b0, b1, b2, a0, a1, bmix = w.bias if bias else (None,) * 6
    return ops.fold_tables(w.E, enc_e, enc_r, t0, w.W0, b0, w.W1, b1, w.W2, b2, w.A0, a0, w.Wmix, bmix, w.A1, w.K, w.nR, aggregates=form == "fold")


def _launch(w, form, ws, items, t0, t1, q, uo, bias, order=None, want_item_emb=True):
    """One launch, run twice: the same bits both times."""
    from mvin_amd import ops
    enc_e, enc_r, _ = _enc(w)
    a1 = w.bias[4] if bias else None
    if form == "fold":
        assert ops.score_l2_folded_supported(w.D, w.K, w.n_entity, w.nR)
        call = lambda: ops.score_l2_folded(ws, enc_e, enc_r, items, t0, t1, q, uo, w.A1, a1, w.Wmix, w.K, w.D, w.nR, w.n_entity,      # noqa: E731
                                           want_item_emb=want_item_emb)
    else:
        assert ops.score_l2_folded_gather_supported(w.D, w.K, w.n_entity, w.nR)
        call = lambda: ops.score_l2_folded_gather(ws, enc_e, enc_r, items, t0, t1, q, uo, w.A1, a1, w.Wmix, w.K, w.D, w.nR, w.n_entity,      # noqa: E731
                                                  order=order, want_item_emb=want_item_emb)
    out, again = call(), call()
    torch.cuda.synchronize()
    for x, y in zip(out, again):
        assert (x is None and y is None) or torch.equal(x, y), "two runs of one launch differ"
    return out


def _references(w, c, t0, t1, bias):
    """-> the float64 and the fp32 evaluation of the reference for the case's pairs, and the yardstick: err_f32 per output over the
    extended set."""
    b0, b1, b2, a0, a1, bmix = w.bias if bias else (None,) * 6
    items, q, uo = c.ext
    args = (w.E, w.ae, w.ar, items, t0, t1, q, uo, w.W0, b0, w.W1, b1, w.W2, b2, w.A0, a0, w.A1, a1, w.Wmix, bmix, w.K)
    r64, r32 = fold_reference(*args)[2:], fold_reference(*args, dtype=torch.float32)[2:]
    yard = [float((b.double() - a).abs().max()) for a, b in zip(r64, r32)]
    return [r[: c.B] for r in r64], [r[: c.B] for r in r32], yard


def _compare(fid, what, got, refs, fails):
    """The relative rule per output, and the tail kernel's absolute bounds where the form's output is held to them."""
    ref64, ref32, yard = refs
    names = ("item_emb", "scores", "sigmoid")
    compare(names, got, ref64, ref32, what, fails, hold_tail=[(fid, n) in TAIL_BOUNDS_HOLD for n in names], stats=STATS, key=fid, yard=yard)


def _report(fid):
    report(STATS, fid)


def _orders(form, items):
    from mvin_amd import ops
    B = items.shape[0]
    if form != "gather" or B == 1:
        return [("as given", None)]
    return [("as given", None), ("key order", ops.order_by_key(items)),
            ("reversed", torch.flip(torch.arange(B, dtype=torch.int32, device=DEV), dims=[0]))]


def _check_tables(w, form, ws, t0, what, fails):
    """TA1 | TA2 | T0A | M0 (and H0 | G of the aggregates form) against their float64 definitions, every row."""
    ref = fold_tables_reference(w.E, w.ae, w.ar, t0, w.W0, w.W1, w.W2, w.A0, w.Wmix, w.K)
    T = ws[: 6 * w.n_entity * w.D].view(6, w.n_entity, w.D).double()
    names = ["TA1", "TA2", "T0A", "M0"] + (["H0", "G"] if form == "fold" else [])
    for i, nm in enumerate(names):
        err = (T[i] - ref[nm]).abs()
        worst = float((err / (2e-5 * ref[nm].abs() + 5e-6)).max())
        if not worst <= 1.0:
            fails.append(f"{what} table {nm}: {worst:.2f} x (rtol 2e-5, atol 5e-6), max abs err {float(err.max()):.3e}")


def _axes(bi, ai, att):
    """The axes that are not crossed, rotated over the crossed ones: every value several times per form."""
    idx = bi * len(ATTENTION) + ai
    return dict(bias=idx % 2 == 0, i64=idx % 4 < 2, pattern=PATTERNS[(idx // 4) % 4], uo_is_q=idx % 3 == 0,
                nR=1 if idx % 7 == 3 and att != "sharp" else 7)


def _run_case(fid, w, kind, c, att, bias, what, fails, tables=False, keep=None):
    """One case: tables (where asked), reference and yardstick once, every order of the launch against them.  ``keep``: a list that
    receives the outputs of every launch."""
    t0, t1 = _logits(w, att)
    ws = _tables(w, kind, t0, bias)
    if tables:
        _check_tables(w, kind, ws, t0, what, fails)
    refs = _references(w, c, t0, t1, bias)
    for oname, order in _orders(kind, c.items):
        got = _launch(w, kind, ws, c.items, t0, t1, c.q, c.uo, bias, order=order)
        _compare(fid, f"{what} order={oname}", got, refs, fails)
        if keep is not None:
            keep.append(got)


@pytest.mark.parametrize("att", ATTENTION)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_batch_size_against_float64(form, att, hip_lib):
    """B x attention crossed fully; biases, id width, item pattern, user_o = q and the relation count rotate over them."""
    kind, D, K = form
    fid = "%s-D%dK%d" % form
    ai = ATTENTION.index(att)
    fails, tables_done = [], set()
    for bi, B in enumerate(batch_sizes(K)):
        ax = _axes(bi, ai, att)
        w = _world(D, K, N_ENTITY, ax["nR"], "counts")
        c = _case(w, ax["pattern"], B, ax["i64"], ax["uo_is_q"], seed=1000 * bi + ai)
        _run_case(fid, w, kind, c, att, ax["bias"], f"{fid} att={att} B={B} {ax}", fails, tables=ax["nR"] not in tables_done)
        tables_done.add(ax["nR"])
    _report(fid)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_item_patterns_against_float64(form, pattern, hip_lib):
    """Runs of one item (1 .. 9 pairs each, sorted), one item for the whole batch, ids out of range: ragged and several-batch launches."""
    kind, D, K = form
    fid = "%s-D%dK%d" % form
    w = _world(D, K, N_ENTITY, 7, "counts")
    fails = []
    for n, (B, att, i64, uo_is_q, bias) in enumerate(pattern_cases(K)):
        c = _case(w, pattern, B, i64, uo_is_q, seed=77 + n, item_seed=n)
        _run_case(fid, w, kind, c, att, bias, f"{fid} {pattern} B={B} att={att} i64={i64} uo_is_q={uo_is_q} bias={bias}", fails)
    _report(fid)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n_entity", [1, 7, 17])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_tables_around_one_tile_of_rows(form, n_entity, hip_lib):
    """Entity tables below and just above the 16 rows of one tile of the table builders (random adjacency), tables and scores."""
    kind, D, K = form
    fid = "%s-D%dK%d" % form
    fails = []
    for n, (B, att, nR, i64, bias) in enumerate(small_table_cases(K)):
        w = _world(D, K, n_entity, nR, "random")
        c = _case(w, "stride" if n % 2 == 0 else "runs", B, i64, n == 3, seed=300 + n)
        _run_case(fid, w, kind, c, att, bias, f"{fid} n_entity={n_entity} B={B} att={att} nR={nR}", fails, tables=True)
    _report(fid)
    assert not fails, "\n".join(fails)


HIGH_WORD_IDS = (2 ** 32 + 5, 2 ** 40 + 3, -2 ** 32)          # int64 ids with a high word: the folded entry points read the LOW word (5, 3, 0)


def out_of_range_ids_check(form, i64):
    """-> the outputs whose bits differ between a batch with ids out of range and the same batch with those ids clamped on the host
    (fold_ref.clamp_ids: the low 32-bit word, unsigned, clamped to n_entity - 1)."""
    kind, D, K = form
    w = _world(D, K, N_ENTITY, 7, "counts")
    B = 4 * K + 37
    bad = _items("oob", B, N_ENTITY, i64)
    good = _items("stride", B, N_ENTITY, i64)
    good[::7] = N_ENTITY - 1
    assert int((bad != good).sum()) == (B + 6) // 7 and (i64 or int((bad == -1).sum()) == (B + 13) // 14)
    if i64:
        high = torch.tensor(HIGH_WORD_IDS * 3, dtype=torch.int64, device=DEV)
        bad[1::7][: len(high)] = high
        good[1::7][: len(high)] = clamp_ids(high, N_ENTITY)
        assert clamp_ids(high, N_ENTITY)[:3].tolist() == [5, 3, 0] and int((bad != good).sum()) == (B + 6) // 7 + len(high)
    assert torch.equal(clamp_ids(bad, N_ENTITY), good.long())
    t0, t1 = _logits(w, "unit")
    c = _case(w, "stride", B, i64, False, seed=5)
    ws = _tables(w, kind, t0, True)
    orders = [None] if kind == "fold" else [None, torch.flip(torch.arange(B, dtype=torch.int32, device=DEV), dims=[0])]
    differ = []
    for order in orders:
        x = _launch(w, kind, ws, bad, t0, t1, c.q, c.uo, True, order=order)
        y = _launch(w, kind, ws, good, t0, t1, c.q, c.uo, True, order=order)
        differ += [nm for nm, a, b in zip(("item_emb", "scores", "sigmoid"), x, y) if not torch.equal(a, b)]
    return differ


@pytest.mark.parametrize("idt", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_out_of_range_ids_equal_the_clamped_ids_bit_for_bit(form, idt, hip_lib):
    """Every 7th id beyond the table (n_entity + 12345; int32: also -1, an unsigned word above every id; int64: also ids with a high word
    set, of which the low word counts): the outputs of the same batch with those ids clamped on the host."""
    differ = out_of_range_ids_check(form, idt == torch.int64)
    assert not differ, f"{differ}: ids out of range are not the clamped ids"


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_scores_do_not_depend_on_want_item_emb(form, hip_lib):
    kind, D, K = form
    w = _world(D, K, N_ENTITY, 7, "counts")
    for B, att, uo_is_q in ((4 * K + 37, "unit", False), (17, "none", True), (1, "sharp", False)):
        t0, t1 = _logits(w, att)
        c = _case(w, "stride", B, True, uo_is_q, seed=9 + B)
        ws = _tables(w, kind, t0, True)
        for _, order in _orders(kind, c.items):
            full = _launch(w, kind, ws, c.items, t0, t1, c.q, c.uo, True, order=order)
            bare = _launch(w, kind, ws, c.items, t0, t1, c.q, c.uo, True, order=order, want_item_emb=False)
            assert bare[0] is None and full[0] is not None
            assert torch.equal(full[1], bare[1]) and torch.equal(full[2], bare[2]), f"B={B} att={att}: scores differ without item_emb"


@pytest.mark.parametrize("att", ["unit", "sharp", "none"])
def test_relation_count_at_the_lds_limit(att, hip_lib):
    """2 600 relations at K = 32: the most the folded form's LDS takes (test_folded_form_with_thousands_of_relations), against float64."""
    from mvin_amd import ops
    D, K, nR, n_entity = 64, 32, 2600, 300
    assert ops.score_l2_folded_supported(D, K, n_entity, nR) and not ops.score_l2_folded_supported(D, K, n_entity, 2800)
    fid = "fold-D64K32"
    w = _world(D, K, n_entity, nR, "random")
    fails = []
    for B, bias, i64 in ((77, False, True), (16, True, False)):
        c = _case(w, "stride", B, i64, B == 77, seed=B)
        _run_case(fid, w, "fold", c, att, bias, f"{fid} nR={nR} att={att} B={B}", fails, tables=True)
    _report(fid)
    assert not fails, "\n".join(fails)
