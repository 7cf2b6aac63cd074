"""-m gpu: the per-level forward kernels on their own -- mvin_linear_fwd (linear_mfma_kernel<D, NE>, linear_kernel<NR>),
mvin_gather_attn_fwd_ex / mvin_agg_fwd_ex (gather_attn_kernel<NR, PRE>), mvin_ripple_attn_fwd_ex, mvin_rel_score, mvin_expand_ids --
through their mvin_amd.ops wrappers against the float64 statements of their contracts in tests/fwd_ref.py (pinned to plain torch
float64 ops by tests/test_fwd_ref_host.py).  Every other module uses these kernels as the EXPECTED value of a fused form.

Every case starts from NaN-filled outputs (ops allocates them with torch.empty, which is made to fill with NaN for the call; a
caller's buffer with a column window is NaN all over and must stay NaN outside the window) and runs twice with equal bits.

EXACT cases.  Small integers (values in [-3, 3], weights in [-2, 2]; the aggregator's weight matrices with 4 non-zeros per column so
that the magnitudes stay small at D = 256) and softmax weights that are exact: uniform logits over a power-of-two count, no logits,
or PLANTED logits (one logit 0, the others in [-1000, -800], so that exp underflows to exactly 0 in float32 and in float64).  Every
partial sum is then a multiple of 1/denominator; ``exact()`` asserts on the reference (magnitude=True) that magnitude x denominator <
2^24 and that the reference is such a multiple before it compares, and then the kernel must equal float64 bit for bit (-0 == 0).
Planted cases also assert, without fwd_ref, that s_out x K / o is the planted row itself.  Planted cases with a fan-out that is no
power of two (s_out is S x fl(1/K): two roundings): probs bit for bit, s_out within 2^-23 relative of row / K, out and Z by the
softmax rule below.

REAL-VALUED cases.  Sums of products (linear out, rel_score): |got - ref| <= (n + 2) 2^-24 magnitude per element, n the number of
terms (bias and row bias counted; ReLU is 1-Lipschitz).  Score: sum_j |u_j| bound_j + (Dout + 2) 2^-24 sum_j |out_j u_j|; sigmoid: a
quarter of that + 2^-22.  Softmax kernels: per output tensor err_hip <= 4 err_f32 + 2e-6, err_f32 = fwd_ref under
precision(float32) against fwd_ref in float64 over at least 256 rows of which the case's are the first.  Logit standard deviation 1
and 8.

Shapes.  linear, matrix cores: all 14 instances x (one full-width source: the ``plain`` staging where Din % 32 == 0, the general loop
at Din = 16 and 48 | NE concatenated | gathered int32 beside a dense source | gathered int64 | bf16 | sum of 2 | sum of 3) x rows
{1, 17, 32, 33, 95}; bias, row bias with rows_per_group {1, 3, rows}, ReLU, a column window, score + sigmoid (eight slab partials at
Dout = 128); nz = 1024 / 3072 with 70 rows (one workgroup per z walks 3 tiles); distinct z strides at nz = 3.  The same cases through
linear_kernel<NR> in ONE child process (MVIN_LINEAR_VALU is read once per process; tests/linear_valu_worker.py): against float64 and,
exact cases, bit-equal to the matrix-core results.  linear, VALU: every NR (Dout 8, 12, 24, 48, 96, 200, 256; 1 and 5) with the same
forms and options, 5 and 8 sources of 16 into 16, identity copies, Dsrc = 4, the score at Dout = Din + 4, rows = 65536 + 33 (the
2048-workgroup grid loops).  Ids outside the table read its LAST row, negative ones too (include/mvin_hip.h, src_rows).
agg / gather_attn: D {4, 8, 12, 16, 24, 36, 64, 100, 128, 256} (24: the list of the issue has no D with NR = 4) x K {1, 3, 8, 64, 65,
130} (+ {5, 8, 9} at D = 256: eight prefetched rows) with T cycling through {1, 7, 8, 9, 37} (8-row tiles; T = 9 as 3 pairs x N = 3),
T = 8197 for every D (32-row tiles, prefetch), T = 32768 + 35 at D = 8 (no prefetch); test_agg_switches_are_met_for_every_dim asserts
that every value of every switch occurs for every D.  ripple: modes 0 / 1 x D {4, 12, 16, 64, 128, 256} x Nm {1, 3, 64, 65, 200} x B
{1, 4, 5}, B = 8195 (grid loop), Nm = 4100 (above 64 KB of LDS).  rel_score: nR {1, 3, 4, 5, 1000} x D {4, 64, 68, 256}.  expand_ids:
levels 0..3 x K {1, 3, 8} x B {1, 257} x int32 / int64 items, items outside the table (int64 >= 2^31, negative) clamped to n_entity - 1
and to 0.  The 65536-block grid cap of expand_level_kernel needs 16.7 M outputs and is deliberately left out.

MEASURED on an MI355X: worst error / bound per kernel and family over all tests (-s prints one line per test, kernel and family;
exact families have no ratio: every one of them was bit-equal).  Softmax families: err_hip / (4 err_f32 + 2e-6).
    kernel                    real out   real score   real sigmoid   exact-case sigmoid (/ 2^-22)
    linear_mfma               0.194      0.024        0.025          0.229
    linear_valu@mfma_shapes   0.194      0.026        0.025          0.229      (the child process)
    linear_valu               0.457      0.085        0.165          0.229
    rel_score                 0.285
    kernel        family   out     probs   S       Z
    agg_gather    std1     0.194   0.030   0.046   0.205
    agg_gather    std8     0.268   0.056   0.071   0.167
    agg_gather    mean     0.212   -       0.076   0.179
    agg_gather    planted  0.191   exact   0.330   0.140       (K not 2^n; S against 1.01 x 2^-23 |row / K|)
    agg_dense     std1     0.218   0.047   0.081   0.092
    agg_dense     std8     0.188   0.065   0.100   0.091
    agg_dense     mean     0.206   -       0.072   0.089
    agg_dense     planted  0.198   exact   0.330   0.048
    ripple o      mode 0: std1 0.142, std8 0.122     mode 1: std1 0.117, std8 0.133, Nm = 4100 0.004
The child's real-valued results against the parent's matrix-core ones: out bit-equal in all 506 cases (not asserted), the score
different in 56 of 56 -- which is how test_the_child_ran_the_other_kernel knows that the child took linear_kernel<NR>.
76 tests (about 4 200 cases with the child's), 13 s as a module on its own (33 s where opening the device took 19 s), of which 2.7 s
are the child process; the longest test body is test_agg_and_gather_attn[256] with 1.4 s.

That the module bites was checked on scratch copies of the library with value-only mutations (every address stays inside its buffer),
all cases but the child's run against each:
  * linear_mfma_kernel<128, NE>: the second slab's bias read from the first slab's columns -- 40 cases fail, all in
    test_linear_mfma[128-1] and [128-2] and every case there that has a bias: exact cases off by up to 4 in 20 - 40 % of the
    elements, real-valued ones at 5.8e3 x the bound.
  * sum_sources staging overwrites where it should add (both kernels) -- 398 cases: every sum2 / sum3 case of every one of the 14
    matrix-core and 9 VALU shapes (16 each) and the 30 summed identity copies; exact cases wrong in 98 - 100 % of the elements (by up
    to 89), real-valued ones at 8e3 - 2e5 x the bound.
  * gather_attn_kernel: psum always K -- 70 cases, in test_agg_and_gather_attn of every D (6 - 9 each): exactly the gather cases with
    logits, Wc, c_child and K > 1 (at K = 1 the mutant computes the same); exact cases wrong in 39 - 54 % of the elements of out,
    real-valued ones with err_hip 1.7 - 3.3 against a bound of a few 1e-6 (2.6e5 - 7e5 x).
  * ripple_attn_kernel: pass 2 gathers score_ids -- all 306 cases of test_ripple_attn fail (planted and uniform ones bit-wise, real
    ones at 1e5 - 2e6 x): even Nm = 1, where the softmax is trivial, returns the wrong row.
  * linear_kernel<NR> score epilogue over Dout - 1 columns -- 84 cases: every score / score_all case of the 9 VALU shapes (8 each) and
    all 12 cases at Dout = Din + 4; exact scores off by up to 114, real-valued ones at 2.4e2 - 1e5 x the bound (Dout = 1: score 0).
No other case failed under any of the five.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import fwd_ref
import linear_valu_worker as lw
from linear_valu_worker import DEV, dev, ints, poisoned_empty, reals, same_bits, to_bf16

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64 = np.float64
STATS = {}


def note(kernel, family, ratio):
    STATS[(kernel, family)] = max(STATS.get((kernel, family), 0.0), float(ratio))


def report(kernel):
    """The worst ratios noted since the last report of this kernel (one test's)."""
    for (k, fam), r in sorted(STATS.items()):
        if k == kernel:
            print(f"MEASURED {k} {fam}: worst error / bound = {STATS.pop((k, fam)):.3f}")


def exact(got, ref, mag, denom, what):
    """got == ref exactly, after checking on the reference that float32 holds every partial sum."""
    ref, mag = np.asarray(ref, F64), np.asarray(mag, F64)
    assert np.all(mag * denom < 2.0 ** 24), f"{what}: case bug: sum|terms| * {denom} = {mag.max() * denom:.4g} >= 2^24"
    assert np.all(np.abs(ref) <= mag), f"{what}: case bug: magnitude below the value"
    assert np.array_equal(ref * denom, np.round(ref * denom)), f"{what}: case bug: reference is not a multiple of 1/{denom}"
    np.testing.assert_array_equal(np.asarray(got, F64).reshape(ref.shape), ref, err_msg=what)


def bounded(got, ref, bound, what, key):
    got, ref = np.asarray(got, F64).reshape(np.shape(ref)), np.asarray(ref, F64)
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    note(key[0], key[1], worst)
    assert np.all(err <= bound), f"{what}: error {err.max():.3e} above its bound (worst ratio {worst:.2f})"


def softmax_rule(got, ref64, ref32, rows, what, key):
    """err_hip (the case's rows) <= 4 err_f32 (all rows of the reference) + 2e-6."""
    ref64, ref32 = np.asarray(ref64, F64), np.asarray(ref32, F64)
    got = np.asarray(got, F64).reshape((rows,) + ref64.shape[1:])
    assert np.isfinite(got).all(), f"{what}: not finite"
    err_hip, err_f32 = float(np.abs(got - ref64[:rows]).max()), float(np.abs(ref32 - ref64).max())
    ratio = err_hip / (4 * err_f32 + 2e-6)
    note(key[0], key[1], ratio)
    assert ratio <= 1.0, f"{what}: err_hip {err_hip:.3e} > 4 x err_f32 {err_f32:.3e} + 2e-6 ({ratio:.2f} x)"


def twice(launch, what):
    """launch() -> tuple of tensors (or None), run twice under poisoned torch.empty: equal bits."""
    first = None
    for _ in range(2):
        with poisoned_empty():
            got = launch()
        torch.cuda.synchronize()
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert (a is None) == (b is None) and (a is None or same_bits(a, b)), f"{what}: two launches differ"
    return first


def host(t):
    return None if t is None else t.detach().cpu().numpy().astype(F64)


# =============================================================================================== linear
def check_linear(case, res, kernel):
    s, what = case.spec, case.name
    assert res["clean"], f"{what}: elements outside the output window were written"
    assert res.get("slabs_equal", True), f"{what}: z slabs of identical problems differ"
    kw = case.ref_kwargs()
    ref, mag = fwd_ref.linear(**kw), fwd_ref.linear(magnitude=True, **kw)
    got = np.asarray(res["out"], F64)
    assert np.isfinite(got).all(), f"{what}: output elements left unwritten (or not finite)"
    if not s["real"]:
        exact(got, ref["out"], mag["out"], 1, what)
        if s["score"]:
            exact(res["score"], ref["score"], mag["score"], 1, what + " score")
            bounded(res["sigmoid"], ref["sigmoid"], 2.0 ** -22, what + " sigmoid", (kernel, "exact sigmoid"))
        return
    bound = (case.terms() + 2) * U * mag["out"]
    bounded(got, ref["out"], bound, what, (kernel, "real out"))
    if s["score"]:
        u = np.abs(np.asarray(case.score_u, F64))
        sb = (u * bound[0]).sum(axis=1) + (s["Dout"] + 2) * U * np.abs(ref["out"][0] * case.score_u).sum(axis=1)
        bounded(res["score"], ref["score"], sb, what + " score", (kernel, "real score"))
        bounded(res["sigmoid"], ref["sigmoid"], sb / 4 + 2.0 ** -22, what + " sigmoid", (kernel, "real sigmoid"))


_MFMA = {}


def mfma_result(name):
    if name not in _MFMA:
        c = lw.Case(name, lw.MFMA_CASES[name])
        _MFMA[name] = (c, lw.run(c))
    return _MFMA[name]


def test_the_general_staging_loop_is_in_the_case_list():
    assert not lw.plain_path(16) and not lw.plain_path(48) and all(lw.plain_path(d) for d in (32, 64, 96, 128, 192, 256))
    for Dout, ne in lw.MFMA_SHAPES:
        assert f"D{Dout}_{ne}x{Dout}_plain_r95_exact" in lw.MFMA_CASES and f"D{Dout}_{ne}x{Dout}_plain_r95_real" in lw.MFMA_CASES
    assert (16, 1) in lw.MFMA_SHAPES and (16, 3) in lw.MFMA_SHAPES and len(lw.MFMA_SHAPES) == 14


@pytest.mark.parametrize("Dout,ne", lw.MFMA_SHAPES)
def test_linear_mfma(Dout, ne, hip_lib):
    assert "MVIN_LINEAR_VALU" not in os.environ, "the default process runs the matrix-core kernel"
    for name in lw.shape_cases(Dout, ne):
        check_linear(*mfma_result(name), "linear_mfma")
    report("linear_mfma")


@pytest.fixture(scope="module")
def valu_results(hip_lib, tmp_path_factory):
    """The cases of MFMA_CASES through linear_kernel<NR>: one child process, once."""
    assert "MVIN_LINEAR_VALU" not in os.environ, "the parent compares against its own matrix-core results"
    path = str(tmp_path_factory.mktemp("linear_valu") / "valu.pkl")
    p = subprocess.run([sys.executable, lw.__file__, path], env=dict(os.environ, MVIN_LINEAR_VALU="1"), stdin=subprocess.DEVNULL,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-4000:]}"
    with open(path, "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("Dout,ne", lw.MFMA_SHAPES)
def test_linear_valu_on_the_mfma_shapes(Dout, ne, valu_results):
    for name in lw.shape_cases(Dout, ne):
        case, m = mfma_result(name)
        v = valu_results[name]
        check_linear(case, v, "linear_valu@mfma_shapes")
        if not case.spec["real"]:
            for k in ("out", "score"):
                assert (v[k] is None) == (m[k] is None) and (v[k] is None or np.array_equal(v[k], m[k])), f"{name}: {k} differs between the kernels"
    report("linear_valu@mfma_shapes")


def test_the_child_ran_the_other_kernel(valu_results):
    """The exact cases are bit-equal between the kernels by construction, so they cannot tell whether the child took
    linear_kernel<NR> at all.  Nor can ``out`` of the real-valued ones: on an MI355X all 506 came out bit-equal too (both kernels
    accumulate an output serially over k = 0 .. Din - 1 from 0 and add the bias last; the 4-deep matrix-core steps round like the
    fmaf chain) -- measured, not asserted.  The SCORE can: linear_kernel sums out_j u_j serially over the Dout columns,
    linear_mfma_kernel sums 16-column slab partials that a cross-lane tree produced."""
    real = [n for n, s in lw.MFMA_CASES.items() if s.get("real")]
    scored = [n for n in real if lw.MFMA_CASES[n].get("score")]
    out_differ = sum(not np.array_equal(valu_results[n]["out"], mfma_result(n)[1]["out"]) for n in real)
    score_differ = sum(not np.array_equal(valu_results[n]["score"], mfma_result(n)[1]["score"]) for n in scored)
    print(f"MEASURED linear_valu@mfma_shapes: real-valued cases that differ in some bit from the matrix-core result: out {out_differ} of {len(real)}, "
          f"score {score_differ} of {len(scored)}")
    assert len(scored) == 4 * len(lw.MFMA_SHAPES)
    assert score_differ > 0, "every real-valued score of the child has the bits of the matrix-core kernel: MVIN_LINEAR_VALU was not honoured"


# (Dout, sources, source width): every NR of linear_kernel (1, 2, 4, 8, 16, 32, 32) and the logit / Nm-wide uses of model.py
VALU_SHAPES = [(8, 2, 8), (12, 2, 8), (24, 2, 12), (48, 2, 24), (96, 2, 48), (200, 2, 100), (256, 4, 64), (1, 2, 8), (5, 3, 4)]
BIG_ROWS = 65536 + 33


def valu_extra_cases():
    c = {}
    for nsrc in (5, 8):                                       # Din / Dout > 4: outside the matrix-core set
        for rows in lw.ROWS:
            for real in (False, True):
                t = "real" if real else "exact"
                c[f"wide{nsrc}_concat_r{rows}_{t}"] = dict(nsrc=nsrc, Dsrc=16, Dout=16, rows=rows, real=real, bias=True)
                c[f"wide{nsrc}_gather_r{rows}_{t}"] = dict(nsrc=nsrc, Dsrc=16, Dout=16, rows=rows, real=real, relu=True,
                                                          gather=["i64" if rows % 2 else "i32"] * nsrc)
    for D in (8, 24, 64):                                     # identity copies (W = NULL)
        for rows in lw.ROWS:
            for tag, opt in (("plain", {}), ("gather32", dict(gather=["i32"])), ("gather64", dict(gather=["i64"], bias=True, relu=True)),
                             ("bf16", dict(gather=["i32"], bf16=True)), ("sum2", dict(nsrc=2, sum=True, rowbias=3)),
                             ("window", dict(off=5, pad=3, gather=["i32"]))):
                for real in (False, True):
                    c[f"copy{D}_{tag}_r{rows}_{'real' if real else 'exact'}"] = dict(dict(nsrc=1, Dsrc=D, Dout=D, rows=rows, identity=True, real=real), **opt)
    for Dsrc, Dout in ((8, 12), (44, 48), (252, 256)):        # the score epilogue at the edge the entry point allows
        for rows in (33, 95):
            for real in (False, True):
                c[f"edge{Dout}_score_r{rows}_{'real' if real else 'exact'}"] = dict(nsrc=1, Dsrc=Dsrc, Dout=Dout, rows=rows, real=real, score=True,
                                                                                bias=True, relu=True)
    for i, Dout in enumerate((8, 12, 24, 48, 96, 200)):       # one per NR: more tiles than the 2048 workgroups of the grid
        c[f"big{Dout}_exact"] = dict(nsrc=1, Dsrc=4, Dout=Dout, rows=BIG_ROWS, bias=True, gather=["i32"] if i % 2 else None, ntab=1000)
    c["big24_real"] = dict(nsrc=1, Dsrc=4, Dout=24, rows=BIG_ROWS, real=True, relu=True)
    return c


VALU_EXTRA = valu_extra_cases()


def _run_valu(cases):
    for name, spec in cases.items():
        c = lw.Case(name, spec)
        assert not in_mfma_set(c), f"{name}: a matrix-core shape in the VALU list"
        check_linear(c, lw.run(c), "linear_valu")


def in_mfma_set(c):
    s = c.spec
    return (not s["identity"]) and s["Dout"] in (16, 32, 64, 128) and c.Din % s["Dout"] == 0 and c.Din // s["Dout"] <= (2 if s["Dout"] == 128 else 4)


@pytest.mark.parametrize("Dout,ne,width", VALU_SHAPES)
def test_linear_valu(Dout, ne, width, hip_lib):
    _run_valu(lw.shape_cases(Dout, ne, width, walk=False))
    report("linear_valu")


@pytest.mark.parametrize("group", ["wide", "copy", "edge", "big"])
def test_linear_valu_extra(group, hip_lib):
    _run_valu({k: v for k, v in VALU_EXTRA.items() if k.startswith(group)})
    report("linear_valu")


@pytest.mark.parametrize("ids64", [False, True])
@pytest.mark.parametrize("kernel", ["mfma", "valu", "copy"])
def test_linear_ids_outside_the_table_read_its_last_row(kernel, ids64, hip_lib):
    """include/mvin_hip.h, src_rows: past the end AND negative -> row src_rows - 1.  Pinned twice: against fwd_ref, and directly
    (W = identity: the output row is the table row)."""
    D = 16 if kernel == "mfma" else 8
    spec = dict(nsrc=1, Dsrc=D, Dout=D, rows=33, gather=["i64" if ids64 else "i32"], bad_ids=True, identity=kernel == "copy")
    c = lw.Case(f"bad_ids_{kernel}_{ids64}", spec)
    if kernel != "copy":
        c.W = np.eye(D, dtype=np.float32).ravel()
    res = lw.run(c)
    check_linear(c, res, "linear_ids")
    ids, ntab = c.ids[0].astype(np.int64), spec.get("ntab", 7)
    outside = (ids < 0) | (ids >= ntab)
    assert outside.sum() == (9 if ids64 else 5) and (ids < 0).sum() >= 2
    np.testing.assert_array_equal(res["out"][0][outside], np.broadcast_to(c.srcs[0][ntab - 1], (outside.sum(), D)))
    np.testing.assert_array_equal(res["out"][0][~outside], c.srcs[0][ids[~outside]])


# =============================================================================================== agg / gather_attn
AGG_D = (4, 8, 12, 16, 24, 36, 64, 100, 128, 256)
AGG_K = (1, 3, 8, 64, 65, 130)
AGG_T = (1, 7, 8, 9, 37)
EXACT_FAMILIES = ("uniform", "none", "planted")


def sparse_ints(rng, Din, Dout, nnz=4):
    """[Din, Dout] with at most nnz non-zeros in [-2, 2] per column."""
    W = np.zeros((Din, Dout), np.float32)
    for j in range(Dout):
        W[rng.choice(Din, min(nnz, Din), replace=False), j] = rng.integers(-2, 3, min(nnz, Din))
    return W


class AggCase(object):
    def __init__(self, D, K, T, N, form, family, logits="rel", wc="none", bagg=True, bf16=False, nE=61, nR=7):
        self.name = f"{form}_D{D}_K{K}_T{T}_N{N}_{family}_{logits}_wc-{wc}_{'b' if bagg else 'nob'}{'_bf16' if bf16 else ''}"
        self.D, self.K, self.T, self.N, self.form, self.family, self.logits, self.wc, self.bf16 = D, K, T, N, form, family, logits, wc, bf16
        rng = np.random.default_rng(lw.zlib.crc32(self.name.encode()))
        assert T % N == 0
        self.real = real = family in ("std1", "std8", "mean")
        self.pow2 = K & (K - 1) == 0
        Tref = self.Tref = -(-max(T, 256) // N) * N
        val = (lambda shape: reals(rng, shape)) if real else (lambda shape: ints(rng, shape, -3, 3))
        wgt = (lambda a, b: reals(rng, (a, b), 1.0 / np.sqrt(a))) if real else (lambda a, b: sparse_ints(rng, a, b))
        att = family not in ("none", "mean")
        kstar = None
        low = lambda shape: -rng.integers(800, 1001, shape).astype(np.float32)      # noqa: E731
        self.table = self.adj_e = self.adj_r = self.node = self.child = self.rel_ids = self.t = None
        if form == "gather":
            self.table = to_bf16(val((nE, D))) if bf16 else val((nE, D))
            self.adj_e = rng.integers(0, nE, (nE, K)).astype(np.int32)
            self.adj_r = rng.integers(1 if family == "planted" else 0, nR, (nE, K)).astype(np.int32)
            self.node = rng.integers(0, nE, Tref).astype(np.int32)
            if family == "planted":
                ks = rng.integers(0, K, nE)
                self.adj_r[np.arange(nE), ks] = 0
                kstar = ks[self.node]
                self.planted_rows = self.table[self.adj_e[self.node, kstar]]
            rel_logits = True
        else:
            self.child = val((Tref * K, D))
            rel_logits = logits == "rel"
            if att and rel_logits:
                self.rel_ids = rng.integers(1 if family == "planted" else 0, nR, (Tref, K)).astype(np.int32)
            if family == "planted":
                kstar = rng.integers(0, K, Tref)
                if rel_logits:
                    self.rel_ids[np.arange(Tref), kstar] = 0
                self.planted_rows = self.child.reshape(Tref, K, D)[np.arange(Tref), kstar]
        if att:
            if rel_logits:
                self.t = {"uniform": np.full(nR, 1.5, np.float32), "planted": np.concatenate([[np.float32(0)], low(nR - 1)]),
                          "std1": reals(rng, nR), "std8": reals(rng, nR, 8.0)}[family]
            elif family == "uniform":
                self.t = np.repeat(ints(rng, (Tref, 1), -5, 5), K, axis=1)           # one constant per task
            elif family == "planted":
                self.t = low((Tref, K))
                self.t[np.arange(Tref), kstar] = 0
            else:
                self.t = reals(rng, (Tref, K), 8.0 if family == "std8" else 1.0)
        self.self_vec = val((Tref, D))
        self.Wc = wgt(D, D) if wc != "none" else None
        self.c_child = val((Tref // N, D)) if wc == "both" else None
        self.Wagg = wgt(D, D)
        self.bagg = val((D,)) if bagg else None

    def ref(self, magnitude=False):
        return fwd_ref.agg(self.self_vec, self.Wagg, self.bagg, self.K, child=self.child, rel_ids=self.rel_ids, table=self.table,
                           adj_entity=self.adj_e, adj_relation=self.adj_r, node_ids=self.node, rel_score=self.t, Wc=self.Wc,
                           c_child=self.c_child, N=self.N, magnitude=magnitude)

    def run(self):
        from mvin_amd import ops
        T, N, K, D = self.T, self.N, self.K, self.D
        d = lambda a: None if a is None else dev(a)                                    # noqa: E731
        sv, Wagg, bagg, t = d(self.self_vec), d(self.Wagg), d(self.bagg), d(None if self.t is None else self.t.ravel())
        if self.form == "gather":
            tab, ae, ar, node, Wc, cc = dev(self.table, self.bf16), d(self.adj_e), d(self.adj_r), d(self.node), d(self.Wc), d(self.c_child)
            launch = lambda: ops.gather_attn_ex(tab, ae, ar, node, t, sv, Wc, cc, Wagg, bagg, T // N, N, K, D)   # noqa: E731
        else:
            child, rel = d(self.child), d(None if self.rel_ids is None else self.rel_ids.ravel())
            launch = lambda: ops.agg_ex(sv, child, rel, t, Wagg, bagg, T // N, N, K, D, want_s=True)           # noqa: E731
        out, probs, S, Z = twice(launch, self.name)
        return {"out": host(out).reshape(T, D), "probs": None if probs is None else host(probs).reshape(T, K), "S": host(S), "Z": host(Z)}

    def check(self):
        got, r64, T, K, what = self.run(), self.ref(), self.T, self.K, self.name
        kernel = "agg_" + self.form
        assert (got["probs"] is None) == (r64["probs"] is None)
        for k, v in got.items():
            assert v is None or np.isfinite(v).all(), f"{what} {k}: elements left unwritten (or not finite)"
        if self.real or not self.pow2:
            with fwd_ref.precision(np.float32):
                r32 = self.ref()
            names = ("out", "Z") if not self.real else ("out", "probs", "S", "Z")
            for k in names:
                if got[k] is not None:
                    softmax_rule(got[k], r64[k], r32[k], T, f"{what} {k}", (kernel, f"{self.family} {k}"))
            if not self.real:          # planted, fan-out no power of two
                assert self.family == "planted"
                np.testing.assert_array_equal(got["probs"], r64["probs"][:T], err_msg=what + " probs")
                assert set(np.unique(got["probs"])) <= {0.0, 1.0}
                want = np.asarray(self.planted_rows[:T], F64) / K
                bounded(got["S"], want, 1.01 * 2.0 ** -23 * np.abs(want), what + " S", (kernel, "planted S (K not 2^n)"))
            return
        mag = self.ref(magnitude=True)
        denom = K * K if self.family == "uniform" else K
        for k in ("out", "S", "Z"):
            exact(got[k], r64[k][:T], mag[k][:T], denom, f"{what} {k}")
        if got["probs"] is not None:
            np.testing.assert_array_equal(got["probs"], r64["probs"][:T], err_msg=what + " probs")
        if self.family == "planted":
            np.testing.assert_array_equal(got["S"] * K, np.asarray(self.planted_rows[:T], F64), err_msg=what + ": s_out * K is not the planted row")


def agg_cases(D):
    """The cases of one D as keyword arguments of AggCase; the switches walk with the index so that
    test_agg_switches_are_met_for_every_dim holds."""
    di = AGG_D.index(D)
    cases = []
    Ks = AGG_K + ((5, 9) if D == 256 else ())            # (8 is in AGG_K)
    for ki, K in enumerate(Ks):
        i = di * 7 + ki
        T = AGG_T[(di + ki) % 5]
        N = 3 if T == 9 else 1
        pow2 = K & (K - 1) == 0
        fams = [EXACT_FAMILIES[i % 3] if pow2 else "planted", "std1", "std8"] + (["mean"] if i % 3 == 0 else [])
        for fi, fam in enumerate(fams):
            j = i + fi
            cases.append(dict(D=D, K=K, T=T, N=N, form="gather", family=fam, wc=("both", "wc", "none")[j % 3], bagg=j % 2 == 0, bf16=j % 4 == 1))
            cases.append(dict(D=D, K=K, T=T, N=N, form="dense", family=fam, logits=("rel", "child")[j % 2], bagg=j % 2 == 1))
    # 32-row tiles with the prefetch (257 tiles: not below the 256 CUs, not above 1024)
    big = dict(D=D, T=8197, N=1)
    cases += [dict(big, K=8, form="gather", family=EXACT_FAMILIES[di % 3], wc="both", bf16=di % 2 == 1),
              dict(big, K=8, form="dense", family=EXACT_FAMILIES[(di + 1) % 3], logits="rel"),
              dict(big, K=3, form="gather", family="std8", wc="both"), dict(big, K=3, form="dense", family="std1", logits="child")]
    if D == 8:                                           # more than 1024 tiles: the instance without the prefetch
        big = dict(D=8, T=32768 + 35, N=1)
        cases += [dict(big, K=3, form="gather", family="std1", wc="both"), dict(big, K=3, form="dense", family="std8"),
                  dict(big, K=8, form="gather", family="planted", wc="wc"), dict(big, K=8, form="dense", family="uniform", logits="child")]
    return cases


def test_agg_switches_are_met_for_every_dim():
    n3 = 0
    for D in AGG_D:
        cs = agg_cases(D)
        small = [c for c in cs if c["T"] <= 37]
        g, d = [c for c in small if c["form"] == "gather"], [c for c in small if c["form"] == "dense"]
        assert {c["K"] for c in small} >= set(AGG_K) and {c["T"] for c in cs} >= set(AGG_T) | {8197}
        assert {c["wc"] for c in g} == {"both", "wc", "none"} and {c["bf16"] for c in g} == {True, False}
        for part in (g, d):
            assert {c["family"] in ("none", "mean") for c in part} == {True, False}                 # rel_score None / given
            assert {c["bagg"] for c in part} == {True, False}
            assert {c["family"] for c in part} >= {"planted", "std1", "std8"}
        assert {c["logits"] for c in d if c["family"] not in ("none", "mean")} == {"rel", "child"}
        n3 += sum(c["N"] == 3 and c["wc"] == "both" for c in g)
    assert n3 >= 3, "c_child[t / N] with N = 3"
    assert {c["T"] for c in agg_cases(8)} >= {32768 + 35}


@pytest.mark.parametrize("D", AGG_D)
def test_agg_and_gather_attn(D, hip_lib):
    for spec in agg_cases(D):
        AggCase(**spec).check()
    report("agg_gather")
    report("agg_dense")


# =============================================================================================== ripple_attn
RIP_D = (4, 12, 16, 64, 128, 256)
RIP_NM = (1, 3, 64, 65, 200)
RIP_B = (1, 4, 5)


class RippleCase(object):
    def __init__(self, D, Nm, B, mode, family, bf16=False, window=False, nE=97, nR=5):
        self.name = f"ripple_D{D}_Nm{Nm}_B{B}_mode{mode}_{family}{'_bf16' if bf16 else ''}{'_window' if window else ''}"
        self.D, self.Nm, self.B, self.mode, self.family, self.bf16, self.nR = D, Nm, B, mode, family, bf16, nR
        rng = np.random.default_rng(lw.zlib.crc32(self.name.encode()))
        self.real = real = family in ("std1", "std8")
        Bref = self.Bref = max(B, 256)
        self.off, self.ldo = (4, D + 8) if window else (0, D)
        E = reals(rng, (nE, D)) if real else ints(rng, (nE, D), -3, 3)
        half = nE // 2
        self.sid = rng.integers(0, nE, (Bref, Nm)).astype(np.int32)
        self.vid = rng.integers(0, nE, (Bref, Nm)).astype(np.int32)
        self.rid = rng.integers(0, nR, (Bref, Nm)).astype(np.int32)
        if real:
            std = (8.0 if family == "std8" else 1.0) / np.sqrt(D)
            self.w, self.V = reals(rng, (3 * D,), std), reals(rng, (Bref, nR, D), std)
        else:
            # logits come from column 0 alone: 0 for the rows below nE / 2 (all rows: uniform; Nm = 1: any integers do)
            self.w, self.V = np.zeros(3 * D, np.float32), np.zeros((Bref, nR, D), np.float32)
            if family == "single":
                assert Nm == 1
                self.w, self.V = ints(rng, (3 * D,), -2, 2), ints(rng, (Bref, nR, D), -2, 2)
            else:
                self.w[0] = 500
                self.V[:, :, 0] = rng.integers(5, 8, (Bref, nR)) * 100
                E[:, 0] = 0
                if family == "planted":
                    E[half:, 0] = -rng.integers(2, 4, nE - half)             # logits <= -1000
                    self.mstar = rng.integers(0, Nm, Bref)
                    self.sid = rng.integers(half, nE, (Bref, Nm)).astype(np.int32)
                    self.sid[np.arange(Bref), self.mstar] = rng.integers(0, half, Bref)
                else:
                    assert family == "uniform" and Nm & (Nm - 1) == 0
        self.E = to_bf16(E) if bf16 else E

    def ref(self, magnitude=False):
        return fwd_ref.ripple_attn(self.E, self.sid, self.vid, self.mode, rel_ids=self.rid, V=self.V, w=self.w, nR=self.nR, magnitude=magnitude)

    def run(self):
        from mvin_amd import ops
        B, D = self.B, self.D
        E, sid, vid = dev(self.E, self.bf16), dev(self.sid[:B]), dev(self.vid[:B])
        rid, V, w = (dev(self.rid[:B]), dev(self.V[:B]), None) if self.mode == 0 else (None, None, dev(self.w))

        def launch():
            buf = torch.full((B, self.ldo), float("nan"), dtype=torch.float32, device=DEV)
            ops.ripple_attn(E, sid, rid, vid, V, w, self.mode, buf, self.off, self.ldo, self.nR)
            return (buf,)

        buf = host(twice(launch, self.name)[0])
        o = buf[:, self.off:self.off + D].copy()
        buf[:, self.off:self.off + D] = np.nan
        assert np.isnan(buf).all(), f"{self.name}: columns outside the window were written"
        assert np.isfinite(o).all(), f"{self.name}: rows left unwritten (or not finite)"
        return o

    def check(self):
        o, r64, B = self.run(), self.ref(), self.B
        if self.real:
            with fwd_ref.precision(np.float32):
                r32 = self.ref()
            softmax_rule(o, r64["o"], r32["o"], B, self.name, ("ripple", f"mode{self.mode} {self.family}"))
            return
        if self.family == "planted":
            assert r64["logits"].max() == 0 and np.sort(r64["logits"], axis=1)[:, :-1].max(initial=-1000) <= -1000
            np.testing.assert_array_equal(o, np.asarray(self.E, F64)[self.vid[np.arange(B), self.mstar[:B]]], err_msg=self.name + ": o is not the planted row")
        exact(o, r64["o"][:B], self.ref(magnitude=True)["o"][:B], self.Nm if self.family == "uniform" else 1, self.name)


def ripple_cases(D):
    cases = []
    for ni, Nm in enumerate(RIP_NM):
        for bi, B in enumerate(RIP_B):
            i = ni + bi
            opt = dict(bf16=i % 3 == 0, window=i % 3 == 1)
            cases += [RippleCase(D, Nm, B, i % 2, "std1", **opt), RippleCase(D, Nm, B, 1 - i % 2, "std8", **opt),
                      RippleCase(D, Nm, B, i % 2, "planted", **opt)]
            if Nm & (Nm - 1) == 0:
                cases.append(RippleCase(D, Nm, B, 1 - i % 2, "single" if Nm == 1 else "uniform", **opt))
    return cases


@pytest.mark.parametrize("D", RIP_D)
def test_ripple_attn(D, hip_lib):
    for c in ripple_cases(D):
        c.check()
    report("ripple")


def test_ripple_attn_grid_loop(hip_lib):
    """8195 pairs: more than the 2048 workgroups x 4 waves of the grid."""
    for mode in (0, 1):
        RippleCase(4, 3, 8195, mode, "std1", window=mode == 1).check()
        RippleCase(4, 3, 8195, mode, "planted", bf16=mode == 0).check()
    report("ripple")


def test_ripple_attn_above_64k_of_lds(hip_lib):
    """Nm = 4100: 4 waves x 4100 logits = 65 600 bytes of dynamic LDS, which needs the opt-in launch_ripple now requests."""
    RippleCase(8, 4100, 3, 1, "std1").check()
    RippleCase(8, 4100, 3, 1, "planted").check()
    report("ripple")


# =============================================================================================== rel_score / expand_ids
@pytest.mark.parametrize("D", [4, 64, 68, 256])
def test_rel_score(D, hip_lib):
    from mvin_amd import ops
    for nR in (1, 3, 4, 5, 1000):
        for real in (False, True):
            what = f"rel_score_nR{nR}_D{D}_{'real' if real else 'exact'}"
            rng = np.random.default_rng(lw.zlib.crc32(what.encode()))
            rel, w = (reals(rng, (nR, D)), reals(rng, (3 * D, 1))) if real else (ints(rng, (nR, D), -3, 3), ints(rng, (3 * D, 1), -2, 2))
            trel, tw = dev(rel), dev(w)
            got = host(twice(lambda: (ops.rel_score(trel, tw),), what)[0])
            ref, mag = fwd_ref.rel_score(rel, w), fwd_ref.rel_score(rel, w, magnitude=True)
            assert np.isfinite(got).all(), f"{what}: rows left unwritten"
            if real:
                bounded(got, ref, (D + 2) * U * mag, what, ("rel_score", "real"))
            else:
                exact(got, ref, mag, 1, what)
    report("rel_score")


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("B", [1, 257])
def test_expand_ids(B, i64, hip_lib):
    from mvin_amd import ops
    nE, nR = 53, 6
    for K in (1, 3, 8):
        for levels in range(4):
            what = f"expand_B{B}_K{K}_L{levels}_{'i64' if i64 else 'i32'}"
            rng = np.random.default_rng(lw.zlib.crc32(what.encode()))
            adj_e, adj_r = rng.integers(0, nE, (nE, K)).astype(np.int32), rng.integers(0, nR, (nE, K)).astype(np.int32)
            items = rng.integers(0, nE, B).astype(np.int64 if i64 else np.int32)
            bad = [-1, nE, nE - 1, 0, -2 ** 31, 2 ** 31 - 1] + ([2 ** 31, 2 ** 31 + 7, 2 ** 40, -2 ** 40] if i64 else [])
            n = min(B, len(bad))
            items[rng.choice(B, n, replace=False)] = bad[:n] if B > 1 else [bad[(K + levels) % len(bad)]]
            te, tr, ti = dev(adj_e), dev(adj_r), dev(items)

            def launch():
                ents, rels = ops.expand_ids(te, tr, ti, K, levels, nE)
                return tuple(ents) + tuple(rels)

            got = [t.cpu().numpy() for t in twice(launch, what)]
            ents, rels = fwd_ref.expand_ids(adj_e, adj_r, items, K, levels, nE)
            assert len(got) == 2 * levels + 1
            for e, (g, r) in enumerate(zip(got, ents + rels)):
                assert g.dtype == np.int32
                np.testing.assert_array_equal(g, r, err_msg=f"{what}: list {e}")
            # the clamp, stated directly: below 0 -> entity 0, at or above n_entity -> n_entity - 1
            want0 = np.where(items.astype(np.int64) < 0, 0, np.minimum(items.astype(np.int64), nE - 1))
            np.testing.assert_array_equal(got[0].ravel(), want0)
