"""-m gpu: first-stage retrieval kernels.  mvin_mips_scores against float64 within a derived bound (bit for bit on integer
inputs); mvin_mips_topk bit for bit against ops.topk_rows on the dense scores, against tests/mips_oracle.py's selection on those
scores and against the composed form of ops.mips_topk, over the shapes of mips_oracle.REAL_CASES, every split count, table
orders that stress pruning, special values, exclusions, candidate ids, strided tables and scales; a query's bits alone, among
300 others and at another tile position; mvin_mean_rows_segments bit for bit for every lane-group width.  Outputs are guarded."""
import numpy as np
import pytest
import torch

import mips_oracle as mo
from mvin_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
PATTERN = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def table(case):
    return dev(case["buf"])[:, :case["D"]]                    # rows ld floats apart


def guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    return whole[GUARD:GUARD + n].view(dtype).view(shape), whole


def intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == PATTERN).all() and (w[-GUARD:] == PATTERN).all())


def csr(excl):
    ptr = np.zeros(len(excl) + 1, np.int64)
    ptr[1:] = np.cumsum([len(e) for e in excl])
    flat = np.concatenate([np.sort(np.fromiter(e, np.int64)) for e in excl] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dev(ptr), dev(flat)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def dense(case, cand=None, off=0, n=None, **kw):
    q = dev(case["q"])
    n_cols = len(cand) if cand is not None else (case["feat"].shape[0] - off if n is None else n)
    out, whole = guarded((q.shape[0], n_cols))
    got = ops.mips_scores(q, table(case), cand_ids=None if cand is None else dev(np.asarray(cand, np.int32)), col_offset=off, n=n,
                          out=out, **kw)
    torch.cuda.synchronize()
    assert intact(whole), "a write outside the score buffer"
    return got


def select(case, k, cand=None, off=0, n=None, excl=None, form="fused", splits=0, **kw):
    """(ids, value bits) of one guarded ops.mips_topk call."""
    q = dev(case["q"])
    (oi, wi), (ov, wv) = guarded((q.shape[0], k), torch.int32), guarded((q.shape[0], k))
    ops.mips_topk(q, table(case), k, cand_ids=None if cand is None else dev(np.asarray(cand, np.int32)), col_offset=off, n=n,
                  excl=None if excl is None else csr(excl), form=form, splits=splits, out=(oi, ov), **kw)
    torch.cuda.synchronize()
    assert intact(wi) and intact(wv), "a write outside an output buffer"
    return oi.cpu().numpy(), bits(ov)


def check_all_forms(case, k, cand=None, off=0, n=None, excl=None, splits=(0,), fused=True, **kw):
    """The dense scores of the case, then: the oracle's selection on them, ops.topk_rows on them (where no column is ineligible),
    the composed form and the fused form for every split count -- all the same ids and value bits."""
    s = dense(case, cand, off, n, **kw)
    sh = s.cpu().numpy()
    n_rows = case["feat"].shape[0]
    rows, elig = mo.row_ids(n_rows, n=sh.shape[1], cand_ids=cand, col_offset=off)
    want = mo.topk(sh, rows, elig, k, excl)
    assert (bits(s) != 0x80000000).all() and (bits(s)[np.isnan(sh)] == mo.QNAN).all()
    if elig.all():
        ti, tv = ops.topk_rows(s, k, cand_ids=None if cand is None else dev(np.asarray(cand, np.int32)), col_offset=off,
                               excl=None if excl is None else csr(excl))
        np.testing.assert_array_equal(ti.cpu().numpy(), want[0])
        np.testing.assert_array_equal(bits(tv), want[1])
    got = select(case, k, cand, off, n, excl, form="composed", max_scores=256 * case["q"].shape[0], **kw)    # blocks of 256 columns
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    for sp in splits if fused else ():
        got = select(case, k, cand, off, n, excl, form="fused", splits=sp, **kw)
        np.testing.assert_array_equal(got[0], want[0], err_msg=f"splits={sp}")
        np.testing.assert_array_equal(got[1], want[1], err_msg=f"splits={sp}")
    return want


# ---------------------------------------------------------------- dense form against float64

@pytest.mark.parametrize("D", [4, 8, 60, 64, 128, 256])
def test_dense_within_the_bound_of_float64(D):
    case = mo.real_case(65, 300, D, seed=D, ld=D + 4)
    cand = np.concatenate([np.arange(299, -1, -1), [-1, 300, 5, 5, -7, 1 << 30]]).astype(np.int32)
    got = dense(case, cand)
    rows, elig = mo.row_ids(300, cand_ids=cand)
    s64, mag = mo.scores64(case["q"], case["feat"], rows, elig)
    g = got.cpu().numpy()
    err = np.abs(g[:, elig].astype(np.float64) - s64[:, elig])
    bound = mo.dot_bound(D, mag[:, elig])
    print(f"D={D}: largest error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert (bits(got)[:, ~elig] == mo.QNAN).all()


@pytest.mark.parametrize("nq,n,D", [(65, 300, 256), (17, 1000, 64), (1, 5, 4)])
def test_dense_integer_inputs_bit_for_bit(nq, n, D):
    case = mo.int_case(nq, n, D, seed=5)
    rows, elig = mo.row_ids(n, n=n)
    s64, _ = mo.scores64(case["q"], case["feat"], rows, elig)
    np.testing.assert_array_equal(bits(dense(case)), mo.canon_bits(s64.astype(np.float32)))


# ---------------------------------------------------------------- fused form against the composed result

@pytest.mark.parametrize("c", mo.REAL_CASES, ids=lambda c: f"nq{c['nq']}-n{c['n']}-D{c['D']}-k{c['k']}")
def test_fused_equals_composed(c):
    assert ops.mips_topk_max_k() == mo.MAX_K
    case = mo.real_case(c["nq"], c["n_rows"], c["D"], c["seed"])
    fused = c["k"] <= mo.MAX_K
    check_all_forms(case, c["k"], off=c["off"], n=c["n"], fused=fused, splits=(0, 1))
    if not fused:                                             # form=None serves k up to 1024 through the composed form
        a = select(case, c["k"], off=c["off"], n=c["n"], form=None)
        b = select(case, c["k"], off=c["off"], n=c["n"], form="composed")
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_every_split_count_gives_the_same_bits():
    case = mo.real_case(40, 2000, 32, seed=9)
    rng = np.random.default_rng(1)
    excl = [sorted(rng.choice(2000, 30, replace=False).tolist()) if i % 2 else [] for i in range(40)]
    check_all_forms(case, 20, excl=excl, splits=(1, 2, 3, 7))
    check_all_forms(case, 20, n=17, splits=(1, 2, 7))          # more ranges than steps: some are empty


@pytest.mark.parametrize("kind", ["ascending", "descending", "equal", "two_values"])
def test_table_orders_that_stress_pruning(kind):
    case, s = mo.order_case(kind, 2000)
    want = check_all_forms(case, 4, splits=(1, 3))
    rows, elig = mo.row_ids(2000, n=2000)
    exact = mo.topk(s, rows, elig, 4)                           # the scores are exact, so the oracle needs no device values
    np.testing.assert_array_equal(want[0], exact[0])
    np.testing.assert_array_equal(want[1], exact[1])
    if kind == "equal":
        assert want[0].tolist() == [[0, 1, 2, 3]] * 3


def test_special_values():
    case = mo.real_case(20, 400, 8, seed=3)
    f = case["buf"]
    f[5, 0], f[6, 1], f[7, 2], f[8] = np.nan, np.inf, -np.inf, 0.0
    f[9] = [np.inf, -np.inf, 0, 0, 0, 0, 0, 0]                  # inf - inf for most queries
    case["q"][3] = 0.0
    case["q"][4] = -0.0                                         # -0.0 products: written as +0.0
    case["q"][5, :] = [0, 0, 0, 1, 0, 0, 0, 0]
    want = check_all_forms(case, 30, splits=(1, 2))
    s = dense(case).cpu().numpy()
    same_sign = case["q"][:, 0] * case["q"][:, 1] > 0          # inf - inf in row 9 for these queries
    assert same_sign.any() and np.isnan(s[same_sign, 9]).all() and np.isinf(s[~same_sign & (case["q"][:, 0] != 0), 9]).all()
    assert np.isnan(s[:, 5]).all() and np.isinf(s[0, 6]) and (s[3] == 0).sum() > 300
    assert want[0][3, :5].tolist() == [0, 1, 2, 3, 4]          # a zero query: the catalogue in order (NaN rows at the end)
    check_all_forms(case, 400, splits=(1,), fused=False)       # every column ranked: NaNs last, in column order


def test_exclusions():
    case = mo.real_case(6, 3000, 8, seed=4)
    rng = np.random.default_rng(2)
    excl = [[], sorted(rng.choice(3000, 40, replace=False).tolist()), list(range(3000)),
            sorted(rng.choice(3000, 2049, replace=False).tolist()), list(range(1, 3000)), [2999]]
    want = check_all_forms(case, 12, excl=excl, splits=(1, 2))
    assert (want[0][2] == -1).all() and want[0][4].tolist() == [0] + [-1] * 11
    assert not set(want[0][3].tolist()) & set(excl[3])


def test_candidate_ids():
    case = mo.real_case(19, 200, 16, seed=6)
    rng = np.random.default_rng(3)
    cand = rng.integers(0, 200, 700)
    cand[::7] = -1
    cand[3::11] = 200 + rng.integers(0, 5, len(cand[3::11]))
    cand[5::13] = -(1 << 31)
    cand[6::17] = (1 << 31) - 1
    assert len(np.unique(cand)) < 250                           # duplicates: every copy is a column of its own
    excl = [sorted(rng.choice(200, 9, replace=False).tolist()) if i % 3 else [] for i in range(19)]
    want = check_all_forms(case, 40, cand=cand.astype(np.int32), excl=excl, splits=(1, 2, 3))
    assert ((want[0] >= 0) & (want[0] < 200)).all()
    few = np.int32([-1, 7, 500, 7, 3])
    want = check_all_forms(case, 5, cand=few, splits=(1,))
    assert (want[0][:, 3:] == -1).all() and (np.sort(want[0][:, :3], axis=1) == [3, 7, 7]).all()


def test_strided_table_and_cosine():
    case = mo.real_case(33, 500, 60, seed=7, ld=72)
    case["buf"][11, :60] = 0.0                                  # a zero row: its inverse norm is 1 / eps
    feat, q = table(case), dev(case["q"])
    rs, qs = ops.row_inv_norms(feat), ops.row_inv_norms(q)
    kw = dict(q_scale=qs, row_scale=rs)
    check_all_forms(case, 25, splits=(1, 2), **kw)
    check_all_forms(case, 25, splits=(1,), q_scale=qs)
    check_all_forms(case, 25, splits=(1,), row_scale=rs)
    got = dense(case, **kw).cpu().numpy().astype(np.float64)
    rows, elig = mo.row_ids(500, n=500)
    s64, mag = mo.scores64(case["q"], case["feat"], rows, elig, qs.cpu().numpy(), rs.cpu().numpy())
    assert (np.abs(got - s64) <= mo.dot_bound(60, mag, n_scales=2)).all()
    # a cosine against the oracle's own norms: sum|q_d e_d| <= |q| |e|, so the dot product's share is gamma_60, each inverse
    # norm is an f64 value rounded once (u each) and each scale product rounds once (u each): (60 + 4) u to first order
    qn, fn = np.linalg.norm(case["q"].astype(np.float64), axis=1), np.linalg.norm(case["feat"].astype(np.float64), axis=1)
    cos = (case["q"].astype(np.float64) @ case["feat"].astype(np.float64).T)[:, fn > 0] / qn[:, None] / fn[None, fn > 0]
    worst = np.abs(got[:, fn > 0] - cos).max()
    print(f"cosine: largest error {worst:.3e}, bound {(60 + 4) * mo.U * 1.01:.3e}")
    assert worst <= (60 + 4) * mo.U * 1.01 and np.abs(got).max() <= 1 + 1e-5


def test_a_query_alone_among_others_and_at_another_position():
    case = mo.real_case(300, 700, 64, seed=8)
    one = dict(case, q=case["q"][37:38].copy())
    moved = dict(case, q=np.concatenate([case["q"][100:123], case["q"][37:38]]))
    a, b, c = dense(case), dense(one), dense(moved)
    np.testing.assert_array_equal(bits(a)[37], bits(b)[0])
    np.testing.assert_array_equal(bits(a)[37], bits(c)[23])
    fa, fb, fc = select(case, 33), select(one, 33, splits=3), select(moved, 33, splits=1)
    for x, y in ((fa[0][37], fb[0][0]), (fa[1][37], fb[1][0]), (fa[0][37], fc[0][23]), (fa[1][37], fc[1][23])):
        np.testing.assert_array_equal(x, y)
    # another column position: the same rows reached through shifted candidate ids
    shifted = dense(case, cand=np.concatenate([[5, 6, 7], np.arange(700)]).astype(np.int32))
    np.testing.assert_array_equal(bits(shifted)[:, 3:], bits(a))


# ---------------------------------------------------------------- the history-mean query

@pytest.mark.parametrize("D,ld", [(4, 4), (64, 64), (60, 68), (256, 256)])
def test_mean_rows_segments_bit_for_bit(D, ld):
    rng = np.random.default_rng(D)
    n_rows = 90
    buf = (rng.standard_normal((n_rows, ld)) * 10.0 ** rng.integers(-3, 4, (n_rows, 1))).astype(np.float32)
    lens = [0, 1, 2, 0, 7, 64, 65, 300, 0, 3] + [int(x) for x in rng.integers(0, 20, 290)]
    ptr = np.zeros(len(lens) + 1, np.int64)
    ptr[1:] = np.cumsum(lens)
    ids = rng.integers(0, n_rows, int(ptr[-1])).astype(np.int32)
    ids[::9] = n_rows + 3
    ids[4::13] = -1
    ids[ptr[9]:ptr[10]] = [-5, n_rows, 1 << 30]                # a segment with nothing inside the table
    want = mo.mean_rows(buf[:, :D], ptr, ids)
    assert not want[9].any() and not want[0].any()
    feat = dev(buf)[:, :D]
    for group in (0, 8, 16, 32, 64):
        out, whole = guarded((len(lens), D))
        ops.mean_rows_segments(feat, dev(ptr), dev(ids), out=out, group=group)
        torch.cuda.synchronize()
        assert intact(whole)
        np.testing.assert_array_equal(bits(out), want.view(np.uint32), err_msg=f"group={group}")
