"""-m gpu: every training kernel of mvin_amd/csrc/mvin_bwd.hip on its own, through its mvin_amd.ops wrapper, against the
float64 statement of its contract in tests/bwd_ref.py (which tests/test_bwd_ref_host.py pins to torch.autograd).

Two families of inputs per kernel.

EXACT cases (coverage, indexing, atomics; the large ones).  Inputs are small integers and every softmax inside a
kernel is uniform over a power-of-two count, so every term and every partial sum, in any order, is a multiple of
1/denominator; float32 holds all of them exactly as long as (sum of |terms|) * denominator < 2^24.  ``exact()`` checks
that condition and the integrality ON THE REFERENCE before it trusts it (a violation is a bug of the case, never a
tolerance), then compares with assert_array_equal: atomics, tile order and MFMA accumulation order cannot matter.

REAL-VALUED cases (arithmetic; short reductions).
  * pure sums of products (weight gradient, scatter-add, count_ids, eltwise 0/2/3/5/6/7/8, L2 without Adam): per output
    element |got - ref| <= (n + 2) * 2^-24 * sum|terms| with n the number of terms: the worst case of any-order float32
    summation of float32 products.  Derived, not measured.  No term is subnormal (|inputs| >= 2^-10).
  * kernels with expf / division / sqrtf inside (agg_bwd with attention, key_addressing_bwd, rel_score_bwd fed by them,
    eltwise 1 and 4, l2_adam_multi with the Adam step): the project's gradient tolerance 2e-4 * max|ref| + 1e-7 per
    output tensor; ``toleranced()`` also evaluates the reference formula in float32 on the CPU and asserts that this
    alone stays within a quarter of the tolerance, so a case the formula itself cannot hold cannot slip in.
"""
import numpy as np
import pytest
import torch

import bwd_ref
from oracle import train_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def ints(rng, shape, lo=-2, hi=2, density=1.0):
    a = rng.integers(lo, hi + 1, shape).astype(np.float32)
    if density < 1.0:
        a *= rng.random(shape) < density
    return a


def reals(rng, shape, scale=1.0):
    """Gaussians with |x| >= 2^-10 * scale: products of two of them are far from subnormal."""
    a = rng.standard_normal(shape)
    a = np.where(np.abs(a) < 2.0 ** -10, np.copysign(2.0 ** -10, a), a)
    return (a * scale).astype(np.float32)


def exact(got, ref, mag, denom, what, prefill=None):
    """got == prefill + ref exactly, after checking on the reference that float32 can hold every partial sum."""
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    if prefill is not None:
        ref, mag = ref + prefill, mag + np.abs(prefill)
    assert np.all(mag * denom < 2.0 ** 24), f"{what}: case bug: sum|terms| * {denom} = {mag.max() * denom:.4g} >= 2^24"
    assert np.all(np.abs(ref) <= mag), f"{what}: case bug: magnitude below the value"
    assert np.array_equal(ref * denom, np.round(ref * denom)), f"{what}: case bug: reference is not a multiple of 1/{denom}"
    np.testing.assert_array_equal(np.asarray(got, np.float64).reshape(ref.shape), ref, err_msg=what)


def summed(got, ref, mag, n, what, prefill=None):
    """Sum-of-products bound: (n + 2) * 2^-24 * sum|terms| per output element."""
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    if prefill is not None:
        ref, mag, n = ref + prefill, mag + np.abs(prefill), n + 1
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    bound = (n + 2) * U * mag
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"  {what}: worst error / bound = {worst:.3f} (n = {n})")
    assert np.all(err <= bound), f"{what}: error {err.max():.3e} above the summation bound (worst ratio {worst:.2f})"


def toleranced(got, ref64, ref32, what):
    """2e-4 * max|ref| + 1e-7 per tensor; the float32 evaluation of the formula itself must stay within a quarter."""
    ref64 = np.asarray(ref64, np.float64)
    tol = 2e-4 * np.abs(ref64).max() + 1e-7
    own = np.abs(np.asarray(ref32, np.float64).reshape(ref64.shape) - ref64).max()
    err = np.abs(np.asarray(got, np.float64).reshape(ref64.shape) - ref64).max()
    print(f"  {what}: gpu {err / tol:.3f} of tolerance, float32 formula {own / tol:.3f}")
    assert own <= 0.25 * tol, f"{what}: case bug: the float32 formula alone is at {own / tol:.2f} of the tolerance"
    assert err <= tol, f"{what}: max abs err {err:.3e} vs tolerance {tol:.3e}"


# =============================================================================================== weight gradient
MFMA_SHAPES = [(1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (4, 2), (6, 2), (8, 2), (4, 4), (8, 4), (12, 4), (16, 4), (8, 8)]
#               Din -> (number of sources, sum them?) so that concat-of-3 and sum-of-2 both occur on the matrix cores
MFMA_SOURCES = {1: (1, False), 2: (1, False), 3: (3, False), 4: (2, True), 6: (3, False), 8: (2, False), 12: (3, False),
                16: (4, False)}
VALU_SHAPES = [  # (nsrc, Dsrc, sum_sources, Dout): Din or Dout not a multiple of 16
    (1, 8, False, 8), (1, 12, False, 16), (1, 16, False, 12), (3, 8, False, 40), (2, 12, True, 24), (1, 40, False, 24),
    (2, 20, False, 5), (1, 40, False, 256), (1, 24, False, 1)]
ROWS = [1, 31, 32, 33, 8191, 8193, 40000, 300000]


class WgradCase(object):
    """One weight-gradient problem: host inputs, device tensors, pre-filled outputs and the reference."""

    def __init__(self, rng, nsrc, Dsrc, sum_sources, Dout, rows, *, nz=1, gathered=None, ids64=False, masked=False,
                 pad=0, want_db=True, real=False, ntab=7):
        self.nsrc, self.Dsrc, self.sum_sources, self.Dout, self.rows, self.nz = nsrc, Dsrc, sum_sources, Dout, rows, nz
        self.Din = Dsrc if sum_sources else nsrc * Dsrc
        gathered = gathered if gathered is not None else [False] * nsrc
        draw = (lambda shape: reals(rng, shape)) if real else (lambda shape: ints(rng, shape))
        self.srcs = [draw((ntab if g else max(rows, 1), Dsrc)) for g in gathered]
        # heavy repeats: a table of ``ntab`` rows feeds every row of X
        self.ids = [rng.integers(0, ntab, max(rows, 1)).astype(np.int64 if ids64 else np.int32) if g else None
                    for g in gathered]
        self.ldy, self.ldm = Dout + pad, Dout + (2 * pad if pad else 0)
        self.dy_zs, self.m_zs = max(rows, 1) * self.ldy + (4 if pad else 0), max(rows, 1) * self.ldm
        self.dY = draw(nz * self.dy_zs)
        self.mask = (rng.integers(-1, 2, nz * self.m_zs).astype(np.float32) if masked else None)   # -1, 0: blocked
        # the kernels ACCUMULATE: integers in the exact cases, values of the size of one term in the real-valued ones
        fill = (lambda shape: reals(rng, shape)) if real else (lambda shape: ints(rng, shape, -50, 50))
        self.dW0 = fill((nz, self.Din, Dout))
        self.db0 = fill((nz, Dout)) if want_db else None
        self.any_ids = any(g for g in gathered)

    def upload(self):
        self.t_srcs = [dev(s) for s in self.srcs]
        self.t_ids = [dev(i) if i is not None else None for i in self.ids] if self.any_ids else None
        self.t_dY, self.t_mask = dev(self.dY), (dev(self.mask) if self.mask is not None else None)
        self.t_dW, self.t_db = dev(self.dW0), (dev(self.db0) if self.db0 is not None else None)
        return self

    def kwargs(self):
        return dict(ids=self.t_ids, db=self.t_db, mask=self.t_mask, sum_sources=self.sum_sources, rows=self.rows,
                    nz=self.nz, ldy=self.ldy, dy_zstride=self.dy_zs, ldm=self.ldm, mask_zstride=self.m_zs,
                    dw_zstride=self.Din * self.Dout, db_zstride=self.Dout)

    def reference(self, magnitude=False):
        if self.rows == 0:
            return np.zeros((self.nz, self.Din, self.Dout)), np.zeros((self.nz, self.Dout))
        return bwd_ref.wgrad(self.srcs, self.dY, self.Dout, ids=self.ids if self.any_ids else None,
                             sum_sources=self.sum_sources, mask=self.mask, rows=self.rows, nz=self.nz, ldy=self.ldy,
                             dy_zstride=self.dy_zs, ldm=self.ldm, mask_zstride=self.m_zs, magnitude=magnitude)

    def check(self, what, real=False):
        (dW, db), (mW, mb) = self.reference(), self.reference(True)
        outputs = [(self.t_dW, dW, mW, " dW", self.dW0)]
        if self.t_db is not None:
            outputs.append((self.t_db, db, mb, " db", self.db0))
        for t, ref, mag, tag, prefill in outputs:
            if real:
                summed(host(t), ref, mag, self.rows, what + tag, prefill)       # one term per row
            else:
                exact(host(t), ref, mag, 1, what + tag, prefill)


def _wgrad_options(i, rows, nsrc):
    """A deterministic walk through the options; test_wgrad_options_meet_the_multi_tile_row_counts asserts that every
    value of every option is met where a workgroup walks more than one row tile."""
    nz = 1 if rows > 40000 else ((1, 3, 12)[i % 3] if rows <= 8193 else (1, 3)[i % 2])
    g = (i // 2) % 4            # 0 dense, 1 all gathered int32, 2 all gathered int64, 3 mixed (int32)
    gathered = [g in (1, 2) or (g == 3 and s % 2 == 1) for s in range(nsrc)]
    return dict(nz=nz, gathered=gathered, ids64=g == 2, masked=i % 2 == 1, pad=(0, 3, 0, 16)[(i // 3) % 4],
                want_db=i % 5 != 4)


def _mfma_option_index(n, ti, tj):
    return n + ti + 2 * tj


def _valu_option_index(n, Dsrc, Dout):
    return n + Dsrc + Dout


def test_wgrad_options_meet_the_multi_tile_row_counts():
    """The coverage table of the exact weight-gradient cases: on the matrix-core kernels and on the VALU kernel alike,
    every value of every option occurs at a row count above 8 192 (several row tiles per workgroup), nz = 12 included."""
    for kernel, indices in (("mfma", [(_mfma_option_index(n, ti, tj), rows, MFMA_SOURCES[ti][0])
                                      for ti, tj in MFMA_SHAPES for n, rows in enumerate(ROWS)]),
                            ("valu", [(_valu_option_index(n, ds, do), rows, ns)
                                      for ns, ds, _, do in VALU_SHAPES for n, rows in enumerate(ROWS)])):
        seen = set()
        for i, rows, nsrc in indices:
            if rows <= 8192:
                continue
            o = _wgrad_options(i, rows, nsrc)
            kind = "dense" if not any(o["gathered"]) else ("int64" if o["ids64"] else
                                                           ("int32" if all(o["gathered"]) else "mixed"))
            seen |= {("nz", o["nz"]), ("ids", kind), ("masked", o["masked"]), ("ldy > Dout", o["pad"] > 0),
                     ("db", o["want_db"])}
        want = {("nz", 1), ("nz", 3), ("nz", 12), ("ids", "dense"), ("ids", "int32"), ("ids", "int64"), ("ids", "mixed"),
                ("masked", False), ("masked", True), ("ldy > Dout", False), ("ldy > Dout", True), ("db", False), ("db", True)}
        assert want <= seen, (kernel, sorted(want - seen, key=str))


@pytest.mark.parametrize("ti,tj", MFMA_SHAPES)
def test_wgrad_mfma_exact(ti, tj, hip_lib):
    """All 13 matrix-core tile shapes at every row count (one row ... 300 000: a workgroup walks many row tiles)."""
    from mvin_amd import ops
    nsrc, sum_sources = MFMA_SOURCES[ti]
    Dsrc = 16 * ti if sum_sources else 16 * ti // nsrc
    rng = np.random.default_rng(1000 + 17 * ti + tj)
    for n, rows in enumerate(ROWS):
        opt = _wgrad_options(_mfma_option_index(n, ti, tj), rows, nsrc)
        c = WgradCase(rng, nsrc, Dsrc, sum_sources, 16 * tj, rows, **opt).upload()
        assert c.Din == 16 * ti
        ops.linear_wgrad(c.t_srcs, c.t_dY, c.t_dW, **c.kwargs())
        c.check(f"mfma {ti}x{tj} rows={rows} {opt}")


@pytest.mark.parametrize("nsrc,Dsrc,sum_sources,Dout", VALU_SHAPES)
def test_wgrad_valu_exact(nsrc, Dsrc, sum_sources, Dout, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(2000 + nsrc * 100 + Dsrc + Dout)
    for n, rows in enumerate(ROWS):
        if rows == 300000 and Dout == 256:
            continue            # 300 000 x 256 gradients: memory, not coverage (40 000 rows already walk 20 tiles each)
        opt = _wgrad_options(_valu_option_index(n, Dsrc, Dout), rows, nsrc)
        c = WgradCase(rng, nsrc, Dsrc, sum_sources, Dout, rows, **opt).upload()
        ops.linear_wgrad(c.t_srcs, c.t_dY, c.t_dW, **c.kwargs())
        c.check(f"valu {nsrc}x{Dsrc}{'+' if sum_sources else '|'}->{Dout} rows={rows} {opt}")


def _multi_cases(rng, spec):
    """spec: list of (nsrc, Dsrc, sum_sources, Dout, rows, nz).  Two identical sets of device buffers."""
    sets = []
    state = rng.bit_generator.state
    for _ in range(2):
        rng.bit_generator.state = state
        sets.append([WgradCase(rng, ns, ds, sm, do, rows, nz=nz, **{k: v for k, v in _wgrad_options(i, max(rows, 1), ns).items()
                                                                    if k != "nz"}).upload()
                     for i, (ns, ds, sm, do, rows, nz) in enumerate(spec)])
    return sets


@pytest.mark.parametrize("name", ["one", "eight", "nine", "twenty", "mixed"])
def test_wgrad_multi_exact_and_equal_to_one_by_one(name, hip_lib):
    """linear_wgrad_multi: 1, 8, 9 and 20 problems of one tile shape (a launch takes 8), and a call that interleaves
    nine problems of one tile shape with three other matrix-core shapes and VALU shapes, different row counts and nz,
    and zero-row problems in the middle."""
    from mvin_amd import ops
    rng = np.random.default_rng(3000 + len(name))
    sizes = [9000, 33, 70000, 1, 4097, 300, 20000, 8193, 2, 64, 12000, 31, 100000, 5, 640, 32, 16385, 7, 2500, 999]
    nzs = [1, 3, 1, 12, 2, 1, 1, 3, 1, 1, 5, 1, 1, 2, 1, 1, 3, 1, 1, 4]
    if name == "mixed":
        spec = [(1, 64, False, 64, 20000, 1), (1, 8, False, 8, 500, 2), (3, 32, False, 32, 9000, 3),
                (1, 64, False, 64, 0, 1), (1, 64, False, 64, 33, 12), (2, 12, True, 24, 4000, 1),
                (3, 32, False, 32, 1, 1), (1, 16, False, 16, 70000, 1), (1, 64, False, 64, 8193, 2),
                (1, 40, False, 24, 0, 3), (3, 32, False, 32, 300, 1), (1, 16, False, 16, 5, 7)]
        # ... and MORE than one launch's worth (nine) of one more tile shape, interleaved with all of the above: the
        # grouping by shape of the entry point together with the chunking into launches of eight
        nine = [(1, 32, False, 32, sizes[i], nzs[i]) for i in range(9)]
        spec = [pr for pair in zip(nine, spec) for pr in pair] + spec[9:]
        assert len(spec) == 21 and sum(pr[:4] == (1, 32, False, 32) for pr in spec) == 9
    else:
        n = {"one": 1, "eight": 8, "nine": 9, "twenty": 20}[name]
        spec = [(1, 32, False, 32, sizes[i], nzs[i]) for i in range(n)]
        if n == 20:
            spec[10] = (1, 32, False, 32, 0, 1)
    multi, single = _multi_cases(rng, spec)
    ops.linear_wgrad_multi([ops.wgrad_problem(c.t_srcs, c.t_dY, c.t_dW, **c.kwargs()) for c in multi])
    for c in single:
        ops.linear_wgrad(c.t_srcs, c.t_dY, c.t_dW, **c.kwargs())
    for i, (cm, cs) in enumerate(zip(multi, single)):
        cm.check(f"multi[{name}] problem {i} {spec[i]}")
        np.testing.assert_array_equal(host(cm.t_dW), host(cs.t_dW), err_msg=f"problem {i}: multi != one by one")
        if cm.t_db is not None:
            np.testing.assert_array_equal(host(cm.t_db), host(cs.t_db), err_msg=f"problem {i}: db multi != one by one")


@pytest.mark.parametrize("nsrc,Dsrc,sum_sources,Dout", [(1, 8, False, 8), (1, 12, False, 16), (1, 16, False, 16),
                                                         (3, 32, False, 32), (2, 64, True, 64), (1, 64, False, 12),
                                                         (2, 32, False, 64), (3, 8, False, 8)])
@pytest.mark.parametrize("rows", [5, 1000, 8192])
def test_wgrad_real_valued(nsrc, Dsrc, sum_sources, Dout, rows, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(4000 + nsrc + Dsrc + Dout + rows)
    opt = _wgrad_options(rows + Dsrc, rows, nsrc)
    opt["nz"] = min(opt["nz"], 3)
    c = WgradCase(rng, nsrc, Dsrc, sum_sources, Dout, rows, real=True, **opt).upload()
    ops.linear_wgrad(c.t_srcs, c.t_dY, c.t_dW, **c.kwargs())
    c.check(f"real {nsrc}x{Dsrc}->{Dout} rows={rows}", real=True)


# =============================================================================================== neighbor mix
def _agg_exact_case(rng, form, T, K, D, nR, n_rows, weights, hot=False, dv_density=0.1):
    """Integer inputs with a uniform (or given dyadic) attention.  Returns (kwargs for bwd_ref.agg_bwd, denominator)."""
    dvec = ints(rng, (T, D), -2, 2, dv_density)
    kw = dict(dvec=dvec)
    if form == "dense":
        kw.update(child=ints(rng, (T * K, D), -1, 1, 0.5), rel_ids=rng.integers(0, nR, T * K).astype(np.int32))
    else:
        hi = 5 if hot else n_rows                       # hot: most tasks hit the same few rows
        adj_e = rng.integers(0, hi, (n_rows, K)).astype(np.int32)
        if hot:
            cold = rng.random((n_rows, K)) < 0.05
            adj_e[cold] = rng.integers(0, n_rows, int(cold.sum()))
        kw.update(table=ints(rng, (n_rows, D), -1, 1, 0.5), adj_entity=adj_e,
                  adj_relation=rng.integers(0, nR, (n_rows, K)).astype(np.int32),
                  node_ids=None if form == "by_entity" else rng.integers(0, n_rows, T).astype(np.int32))
        if form == "by_entity":
            kw["dvec"][rng.random(T) < 0.9] = 0.0       # most rows zero: skipped
    if weights == "uniform":                            # equal scores: softmax = 1/K exactly
        kw["rel_score"] = np.full(nR, 3.0, np.float32)
        denom = K ** 3
    elif weights == "given16":                          # multiples of 1/16 (they need not sum to one for the contract)
        kw["probs"] = (rng.integers(0, 17, (T, K)) / 16.0).astype(np.float32)
        denom = 256 * K
    else:
        denom = K
    if weights == "none":
        kw.pop("rel_ids", None)
        if form != "dense":
            kw["adj_relation"] = None
    return kw, denom


def _run_agg(ops, kw, K, nR, prefill_rng=None):
    """The kernel on the case ``kw`` -> dict like bwd_ref.agg_bwd's (and the pre-filled values)."""
    dvec = kw["dvec"]
    T, D = dvec.shape
    t = {k: (dev(v) if v is not None else None) for k, v in kw.items()}
    att = kw.get("probs") is not None or kw.get("rel_score") is not None
    dT0 = ints(prefill_rng, nR, -8, 8) if att else None
    dT = dev(dT0) if att else None
    out, pre = {}, {"dT": dT0}
    if kw.get("table") is not None:
        pre["dtable"] = ints(prefill_rng, kw["table"].shape, -8, 8)
        dtab = dev(pre["dtable"])
        uses_score_in_kernel = kw.get("probs") is None and kw.get("rel_score") is not None
        if uses_score_in_kernel and kw["node_ids"] is not None:
            pytest.fail("case bug: rel_score in the kernel is the by-entity form")
        ops.agg_bwd(t["dvec"], t.get("probs"), T, K, D, nR, table=t["table"], adj_entity=t["adj_entity"],
                    adj_relation=t.get("adj_relation"), node_ids=t.get("node_ids"), dtable=dtab, dT=dT,
                    rel_score=t.get("rel_score") if uses_score_in_kernel else None)
        out["dtable"] = host(dtab)
    else:
        out["dchild"] = host(ops.agg_bwd(t["dvec"], t.get("probs"), T, K, D, nR, child=t["child"],
                                         rel_ids=t.get("rel_ids"), dT=dT))
    out["dT"] = host(dT) if att else None
    return out, pre


def _agg_with_probs(kw):
    """The dense and node-list forms take probabilities, not scores: hand the kernel the softmax the case stands for."""
    kw = dict(kw)
    if kw.get("rel_score") is not None and not (kw.get("table") is not None and kw.get("node_ids") is None):
        if kw.get("table") is not None:
            rel = kw["adj_relation"][kw["node_ids"].astype(np.int64)]
        else:
            rel = kw["rel_ids"].reshape(kw["dvec"].shape[0], -1)
        kw["probs"] = bwd_ref.softmax(kw.pop("rel_score")[rel]).astype(np.float32)
    return kw


AGG_EXACT = [  # form, T, K, D, nR, n_rows, weights, hot
    ("dense", 1, 8, 16, 4, 0, "uniform", False), ("dense", 5, 64, 128, 9, 0, "uniform", False),
    ("dense", 16385, 16, 32, 64, 0, "given16", False), ("dense", 200000, 8, 16, 64, 0, "uniform", False),
    ("dense", 5, 32, 64, 3, 0, "none", False), ("dense", 16385, 8, 128, 5, 0, "none", False),
    ("gather", 1, 16, 64, 4, 50, "given16", False), ("gather", 5, 8, 128, 4, 50, "uniform", False),
    ("gather", 16385, 32, 64, 12, 3000, "uniform", False), ("gather", 200000, 8, 32, 64, 20011, "given16", True),
    ("gather", 16385, 16, 128, 7, 500, "none", True), ("gather", 200000, 8, 16, 12, 20011, "uniform", True),
    ("gather", 5, 64, 16, 3, 40, "uniform", False),
    ("by_entity", 20011, 8, 64, 12, 20011, "uniform", False), ("by_entity", 200000, 16, 16, 64, 200000, "uniform", False),
    ("by_entity", 5, 32, 32, 4, 5, "uniform", False), ("by_entity", 16385, 64, 128, 9, 16385, "uniform", True),
    ("by_entity", 1, 8, 16, 2, 1, "uniform", False),
]


@pytest.mark.parametrize("form,T,K,D,nR,n_rows,weights,hot", AGG_EXACT)
def test_agg_bwd_exact(form, T, K, D, nR, n_rows, weights, hot, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(5000 + T % 1000 + K + D)
    kw, denom = _agg_exact_case(rng, form, T, K, D, nR, n_rows, weights, hot, dv_density=0.1 if T < 100000 else 0.03)
    kw = _agg_with_probs(kw)
    got, pre = _run_agg(ops, kw, K, nR, rng)
    ref, mag = bwd_ref.agg_bwd(K=K, nR=nR, **kw), bwd_ref.agg_bwd(K=K, nR=nR, magnitude=True, **kw)
    what = f"agg_bwd {form} T={T} K={K} D={D} {weights}"
    if form == "dense":
        exact(got["dchild"], ref["dchild"], mag["dchild"], denom, what + " dchild")
    else:
        exact(got["dtable"], ref["dtable"], mag["dtable"], denom, what + " dtable", pre["dtable"])
    if weights == "none":
        assert got["dT"] is None and ref["dT"] is None
    else:
        exact(got["dT"], ref["dT"], mag["dT"], denom, what + " dT", pre["dT"])


@pytest.mark.parametrize("form", ["dense", "gather", "by_entity"])
@pytest.mark.parametrize("K,D,nR", [(3, 8, 4), (5, 12, 7), (12, 16, 5), (8, 32, 12), (5, 64, 3)])
def test_agg_bwd_and_rel_score_bwd_real_valued(form, K, D, nR, hip_lib):
    """Non-uniform softmaxes over fan-outs that are not powers of two; dT then goes on through rel_score_bwd."""
    from mvin_amd import ops
    rng = np.random.default_rng(6000 + K + D)
    T, n_rows = (300, 300) if form == "by_entity" else (300, 80)
    kw = dict(dvec=reals(rng, (T, D)))
    if form == "dense":
        kw.update(child=reals(rng, (T * K, D)), rel_ids=rng.integers(0, nR, T * K).astype(np.int32))
    else:
        kw.update(table=reals(rng, (n_rows, D)), adj_entity=rng.integers(0, n_rows, (n_rows, K)).astype(np.int32),
                  adj_relation=rng.integers(0, nR, (n_rows, K)).astype(np.int32),
                  node_ids=None if form == "by_entity" else rng.integers(0, n_rows, T).astype(np.int32))
    kw["rel_score"] = reals(rng, nR)
    kw = _agg_with_probs(kw)
    got, pre = _run_agg(ops, kw, K, nR, rng)
    ref = bwd_ref.agg_bwd(K=K, nR=nR, **kw)
    with bwd_ref.precision(np.float32):
        r32 = bwd_ref.agg_bwd(K=K, nR=nR, **kw)
    what = f"agg_bwd real {form} K={K} D={D}"
    key = "dchild" if form == "dense" else "dtable"
    toleranced(got[key] - (pre[key] if key in pre else 0), ref[key], r32[key], what + " " + key)
    toleranced(got["dT"] - pre["dT"], ref["dT"], r32["dT"], what + " dT")
    # rel_score backward on that dT (a pure sum of products over nR terms)
    rel, urh, dT = reals(rng, (nR, D)), reals(rng, 3 * D), (got["dT"] - pre["dT"]).astype(np.float32)
    drel0, durh0 = reals(rng, (nR, D)), reals(rng, 3 * D)
    t_drel, t_durh = dev(drel0), dev(durh0)
    ops.rel_score_bwd(dev(rel), dev(urh), dev(dT), t_drel, t_durh)
    (drel, durh), (mrel, murh) = bwd_ref.rel_score_bwd(rel, urh, dT), bwd_ref.rel_score_bwd(rel, urh, dT, magnitude=True)
    summed(host(t_drel), drel, mrel, 1, what + " drel", drel0)
    summed(host(t_durh), durh, murh, nR, what + " durh", durh0)


# =============================================================================================== key addressing
def _ka_exact_case(rng, D, Nm, P, has_set, B, nE, nR, j, l2, *, one_row_pair=True, e_density=0.1, do_density=0.1,
                   item_share=False):
    """Every logit of a read is the same number: V[b, r] = s_b e_j, w = -2 e_j, and every table row has component j
    equal to 1 (the other components are sparse in {-1, 0, 1}); the softmaxes are then exactly 1 / n_memory."""
    E = ints(rng, (nE, D), -1, 1, e_density)
    E[:, j] = 1.0
    V = np.zeros((B, nR, D), np.float32)
    V[:, :, j] = rng.choice([1.0, 2.0, -1.0], B)[:, None]
    w = None
    if has_set:
        w = np.zeros(D, np.float32)
        w[j] = -2.0
    nh = max(1, P)
    mh = [rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(nh)]
    mr = [rng.integers(0, nR, (B, Nm)).astype(np.int32) for _ in range(P)]
    mt = [rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(P)]
    if one_row_pair:                                     # all memories of a pair on one row (and one relation)
        b = B // 2
        for a in mh + mt:
            a[b, :] = 3 % nE
        for a in mr:
            a[b, :] = nR - 1
    nslot = P + (1 if has_set else 0)
    ldo = nslot * D + (8 if B > 1 else 0)
    dout = ints(rng, B * ldo, -2, 2, do_density)
    kw = dict(E=E, V=V if P else None, w=w, mem_h=mh, mem_r=mr, mem_t=mt, P=P, dout=dout, ldo=ldo, nR=nR, l2=l2)
    if item_share:
        kw.update(relation_kge=ints(rng, (nR, D, D), -1, 1, 0.1), items=rng.integers(0, nE, B))
    return kw


def _run_ka(ops, kw, dw_rep, prefill_rng, items_dtype=np.int64):
    E = kw["E"]
    nE, D = E.shape
    B, P, nR = kw["mem_h"][0].shape[0], kw["P"], kw["nR"]
    pre = {"dE": ints(prefill_rng, (nE, D), -4, 4), "dV": ints(prefill_rng, (B, nR, D), -4, 4) if P else None,
           "reg": np.float64(7.0)}
    dE, dV = dev(pre["dE"]), (dev(pre["dV"]) if P else None)
    dw = torch.zeros((dw_rep, D), dtype=torch.float32, device=DEV) if kw["w"] is not None else None
    reg = torch.full((1,), 7.0, dtype=torch.float32, device=DEV)
    share = kw.get("relation_kge") is not None
    ops.key_addressing_bwd(dev(E), dev(kw["V"]) if P else None, dev(kw["w"]) if kw["w"] is not None else None,
                           [dev(m) for m in kw["mem_h"]], [dev(m) for m in kw["mem_r"]], [dev(m) for m in kw["mem_t"]],
                           P, dev(kw["dout"]), kw["ldo"], nR, kw["l2"], dE, dV, dw, reg_accum=reg,
                           relation_kge=dev(kw["relation_kge"]) if share else None,
                           items=dev(kw["items"], items_dtype) if share else None)
    return {"dE": host(dE), "dV": host(dV) if P else None, "dw_replicas": host(dw) if dw is not None else None,
            "reg": host(reg)[0]}, pre


KA_EXACT = [  # D, Nm, P, has_set, B, nE, nR, j, l2, dw_rep, item_share
    (16, 1, 1, True, 1, 50, 3, 0, 0.5, 1, False), (16, 16, 0, True, 40, 400, 3, 5, 0.5, 1, False),
    (16, 32, 2, False, 40, 3000, 5, 15, 0.25, 1, True), (16, 128, 1, True, 40, 8000, 4, 9, 0.25, 64, False),
    (32, 16, 3, True, 2048, 30011, 12, 31, 0.5, 64, True), (32, 64, 2, True, 40, 6000, 7, 2, 0.25, 64, False),
    (32, 32, 1, False, 5000, 30011, 12, 17, 0.5, 1, False), (32, 1, 2, True, 40, 300, 3, 8, 0.5, 1, True),
    (64, 16, 2, True, 5000, 50021, 12, 63, 0.5, 64, True), (64, 32, 3, False, 2048, 50021, 9, 40, 0.25, 1, True),
    (64, 64, 1, True, 40, 5000, 5, 1, 0.25, 1, False), (64, 128, 2, False, 40, 20011, 12, 33, 0.25, 1, True),
    (64, 16, 1, True, 5000, 50021, 136, 20, 0.5, 64, False),      # 136 relations at dim 64: dV through global memory
    (64, 32, 2, True, 40, 5000, 200, 7, 0.25, 1, False),          # the same, several passes of memories
    (32, 16, 0, True, 5000, 30011, 1, 11, 0.5, 64, False), (16, 64, 3, True, 2048, 30011, 5, 3, 0.5, 64, True),
    (64, 32, 1, True, 1, 200, 3, 62, 0.5, 1, True),
]


@pytest.mark.parametrize("D,Nm,P,has_set,B,nE,nR,j,l2,dw_rep,item_share", KA_EXACT)
def test_key_addressing_bwd_exact(D, Nm, P, has_set, B, nE, nR, j, l2, dw_rep, item_share, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(7000 + D + Nm + P + B % 1000)
    in_kernel = item_share and ops.key_addressing_bwd_adds_item_grad(P, Nm, D, nR)
    assert in_kernel == item_share, "case bug: the item share was asked for at a shape the kernel does not take it at"
    kw = _ka_exact_case(rng, D, Nm, P, has_set, B, nE, nR, j, l2, item_share=item_share,
                        do_density=0.1 if B < 2048 else 0.05, one_row_pair=Nm * max(P, 1) <= 128)
    got, pre = _run_ka(ops, kw, dw_rep, rng, np.int64 if B % 2 else np.int32)
    ref, mag = bwd_ref.key_addressing_bwd(**kw), bwd_ref.key_addressing_bwd(magnitude=True, **kw)
    what = f"key_addressing_bwd D={D} Nm={Nm} P={P} set={has_set} B={B} nR={nR}"
    denom = 4 * Nm * Nm
    exact(got["dE"], ref["dE"], mag["dE"], denom, what + " dE", pre["dE"])
    if P:
        exact(got["dV"], ref["dV"], mag["dV"], denom, what + " dV", pre["dV"])
        exact(got["reg"], ref["reg"], mag["reg"], 4, what + " reg", pre["reg"])
    else:
        assert got["reg"] == 7.0
    if has_set:
        # every replica is a partial sum of the same terms (checked exactly representable below); the caller sums them
        exact(got["dw_replicas"].sum(axis=0), ref["dw"], mag["dw"], denom, what + " dw")
        if dw_rep > 1 and B >= 40:
            assert np.count_nonzero(np.abs(got["dw_replicas"]).sum(axis=1)) > 1, "one replica took everything"


@pytest.mark.parametrize("D", [16, 32, 64])
def test_key_addressing_bwd_exact_every_column(D, hip_lib):
    """In the exact cases V[b, r] = s_b e_j and w = -2 e_j: the dl * V and dl' * w terms of dE live in column j alone.
    One small case (40 pairs, 16 memories, one hop and the h-set read) for EVERY j in range(D), so that every float4
    component of the V read and of the w read carries those terms exactly somewhere."""
    from mvin_amd import ops
    seen = set()
    for j in range(D):
        rng = np.random.default_rng(7500 + 100 * D + j)
        item_share = j % 2 == 0
        nR = 3 + j % 3
        assert ops.key_addressing_bwd_adds_item_grad(1, 16, D, nR)
        kw = _ka_exact_case(rng, D, 16, 1, True, 40, 600, nR, j, 0.5, item_share=item_share)
        got, pre = _run_ka(ops, kw, 1 if j % 4 else 4, rng)
        ref, mag = bwd_ref.key_addressing_bwd(**kw), bwd_ref.key_addressing_bwd(magnitude=True, **kw)
        # the terms this case is for are there: without them column j of dE would be another number
        no_v = bwd_ref.key_addressing_bwd(**dict(kw, V=np.zeros_like(kw["V"]), w=np.zeros_like(kw["w"])))
        assert np.any(no_v["dE"][:, j] != ref["dE"][:, j]), f"case bug: column {j} does not carry the dl * V term"
        what = f"key_addressing_bwd D={D} every column j={j}"
        exact(got["dE"], ref["dE"], mag["dE"], 4 * 16 * 16, what + " dE", pre["dE"])
        exact(got["dV"], ref["dV"], mag["dV"], 4 * 16 * 16, what + " dV", pre["dV"])
        exact(got["reg"], ref["reg"], mag["reg"], 4, what + " reg", pre["reg"])
        exact(got["dw_replicas"].sum(axis=0), ref["dw"], mag["dw"], 4 * 16 * 16, what + " dw")
        seen.add(j)
    assert seen == set(range(D))


@pytest.mark.parametrize("D,Nm,P,has_set,nR,item_share", [(8, 3, 1, True, 4, False), (12, 5, 2, True, 3, True),
                                                          (16, 12, 3, False, 5, True), (32, 5, 1, True, 12, False),
                                                          (64, 12, 2, True, 7, True), (16, 3, 0, True, 1, False),
                                                          (64, 40, 2, True, 140, False)])
def test_key_addressing_bwd_real_valued(D, Nm, P, has_set, nR, item_share, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(8000 + D + Nm + P)
    B, nE, l2 = 64, 500, 1e-3
    nh = max(1, P)
    kw = dict(E=reals(rng, (nE, D), 0.5), V=reals(rng, (B, nR, D), 0.5) if P else None,
              w=reals(rng, D, 0.5) if has_set else None,
              mem_h=[rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(nh)],
              mem_r=[rng.integers(0, nR, (B, Nm)).astype(np.int32) for _ in range(P)],
              mem_t=[rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(P)], P=P, nR=nR, l2=l2)
    kw["ldo"] = (P + (1 if has_set else 0)) * D + 4
    kw["dout"] = reals(rng, B * kw["ldo"])
    if item_share:
        assert ops.key_addressing_bwd_adds_item_grad(P, Nm, D, nR)
        kw.update(relation_kge=reals(rng, (nR, D, D), 0.2), items=rng.integers(0, nE, B))
    got, pre = _run_ka(ops, kw, 4, rng)
    ref = bwd_ref.key_addressing_bwd(**kw)
    with bwd_ref.precision(np.float32):
        r32 = bwd_ref.key_addressing_bwd(**kw)
    what = f"key_addressing_bwd real D={D} Nm={Nm} P={P}"
    toleranced(got["dE"] - pre["dE"], ref["dE"], r32["dE"], what + " dE")
    if P:
        toleranced(got["dV"] - pre["dV"], ref["dV"], r32["dV"], what + " dV")
        toleranced(got["reg"] - pre["reg"], ref["reg"], r32["reg"], what + " reg")
    if has_set:
        toleranced(got["dw_replicas"].sum(axis=0), ref["dw"], r32["dw"], what + " dw")


# =============================================================================================== small kernels
@pytest.mark.parametrize("idt", [np.int32, np.int64])
@pytest.mark.parametrize("rows,D,n_rows,alpha", [(1, 4, 3, 1.0), (70000, 64, 20011, -2.0), (70000, 64, 1, 1.0),
                                                 (300000, 16, 7, 0.5), (5, 128, 9, 4.0)])
def test_scatter_add_rows_exact(idt, rows, D, n_rows, alpha, hip_lib):
    """70 000 x 64 and 300 000 x 16 are above 4 M elements (the grid-stride loop); n_rows = 1: all rows onto one."""
    from mvin_amd import ops
    rng = np.random.default_rng(9000 + rows % 1000 + D)
    ids, x = rng.integers(0, n_rows, rows).astype(idt), ints(rng, (rows, D), -2, 2)
    pre = ints(rng, (n_rows, D), -9, 9)
    t = dev(pre)
    ops.scatter_add_rows(t, dev(ids), dev(x), alpha)
    exact(host(t), bwd_ref.scatter_add_rows(n_rows, ids, x, alpha), bwd_ref.scatter_add_rows(n_rows, ids, x, alpha, True),
          2, f"scatter_add_rows {rows}x{D} -> {n_rows}", pre)


@pytest.mark.parametrize("idt", [np.int32, np.int64])
def test_scatter_add_rows_real_valued(idt, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(9100)
    rows, D, n_rows, alpha = 8192, 12, 3, 0.37
    ids, x = rng.integers(0, n_rows, rows).astype(idt), reals(rng, (rows, D))
    t = torch.zeros((n_rows, D), dtype=torch.float32, device=DEV)
    ops.scatter_add_rows(t, dev(ids), dev(x), alpha)
    a32 = float(np.float32(alpha))
    n = int(np.bincount(ids).max())
    summed(host(t), bwd_ref.scatter_add_rows(n_rows, ids, x, a32), bwd_ref.scatter_add_rows(n_rows, ids, x, a32, True), n,
           "scatter_add_rows real")


@pytest.mark.parametrize("n,nbins", [(1, 1), (5000, 1), (100, 4096), (1500000, 4096), (1500000, 9), (1500000, 4095)])
def test_count_ids_exact(n, nbins, hip_lib):
    """Ids below 0 and at / above nbins are ignored; above 1 M ids the workgroups stride; ``out`` is accumulated into."""
    from mvin_amd import ops
    rng = np.random.default_rng(9200 + n % 100 + nbins)
    ids = rng.integers(-2, nbins + 2, n).astype(np.int32)
    ids[rng.random(n) < 0.3] = 0                    # bin 0 is well filled (and the edges of the range are hit)
    ids[::7] = nbins - 1
    ids[3::11] = nbins
    ids[5::13] = -1
    pre = ints(rng, nbins, 0, 5)
    out = ops.count_ids(dev(ids), nbins, out=dev(pre))
    ref = bwd_ref.count_ids(ids, nbins)
    assert ref[0] > 0 and ref[nbins - 1] > 0
    exact(host(out), ref, ref, 1, f"count_ids n={n} nbins={nbins}", pre)
    fresh = ops.count_ids(dev(ids), nbins)
    exact(host(fresh), ref, ref, 1, f"count_ids n={n} nbins={nbins} (fresh out)")


BIG = 4 * 1024 * 1024 + 4096 * 3 + 64      # above 4 M elements: every eltwise grid strides, with a ragged end


@pytest.mark.parametrize("mode", [0, 2, 3, 5, 6, 7, 8])
def test_eltwise_exact(mode, hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(9300 + mode)
    D = 64
    n = BIG if mode in (0, 2, 3) else (BIG // D) * D
    rows = n // D
    acc0 = 5.0
    acc = torch.full((1,), acc0, dtype=torch.float32, device=DEV)
    if mode == 0:
        x, y = ints(rng, n), ints(rng, n)
        for alpha, beta in ((2.0, -0.5), (-1.0, 0.0)):
            ty = dev(y)
            ops.eltwise(0, n, dev(x), ty, alpha=alpha, beta=beta)
            exact(host(ty), bwd_ref.eltwise(0, x, y, alpha=alpha, beta=beta)["y"],
                  bwd_ref.eltwise(0, x, y, alpha=alpha, beta=beta, magnitude=True)["y"], 2, f"eltwise 0 beta={beta}")
        ty = dev(y)
        assert ops.axpby(3.0, dev(x), 1.0, ty) is ty
        exact(host(ty), 3.0 * x.astype(np.float64) + y, 3.0 * np.abs(x) + np.abs(y), 1, "axpby")
    elif mode == 2:
        x, z = ints(rng, n), ints(rng, n, -1, 1)
        ty = torch.full((n,), 9.0, dtype=torch.float32, device=DEV)
        ops.eltwise(2, n, dev(x), ty, dev(z))
        exact(host(ty), bwd_ref.eltwise(2, x, z=z)["y"], np.abs(x), 1, "eltwise 2")
    elif mode == 3:
        x = ints(rng, n, -1, 1)
        ops.eltwise(3, n, dev(x), accum=acc, alpha=0.5)
        r = bwd_ref.eltwise(3, x, alpha=0.5)["accum"]
        exact(host(acc)[0], r, r, 2, "eltwise 3", acc0)
    elif mode == 5:
        x, y, z = ints(rng, n), ints(rng, n), ints(rng, rows, -3, 3)
        for beta in (0.0, 2.0):
            ty = dev(y)
            ops.eltwise(5, n, dev(x), ty, dev(z), alpha=0.5, beta=beta, D=D)
            exact(host(ty), bwd_ref.eltwise(5, x, y, z, alpha=0.5, beta=beta, D=D)["y"],
                  bwd_ref.eltwise(5, x, y, z, alpha=0.5, beta=beta, D=D, magnitude=True)["y"], 2, f"eltwise 5 beta={beta}")
    elif mode == 6:
        for N, Dg in ((3, 64), (8, 64), (21, 16), (1, 64)):
            groups = min(BIG // Dg, (24 * 1024 * 1024) // (N * Dg))     # groups * D outputs, N rows each
            x = ints(rng, groups * N * Dg)
            ty = torch.full((groups * Dg,), 9.0, dtype=torch.float32, device=DEV)
            ops.eltwise(6, groups * Dg, dev(x), ty, alpha=-0.5, D=Dg, N=N)
            exact(host(ty), bwd_ref.eltwise(6, x, alpha=-0.5, D=Dg, N=N)["y"],
                  bwd_ref.eltwise(6, x, alpha=-0.5, D=Dg, N=N, magnitude=True)["y"], 2, f"eltwise 6 N={N} D={Dg}")
    elif mode == 7:
        x, z = ints(rng, n, -1, 1), ints(rng, rows, -2, 2)
        ops.eltwise(7, n, dev(x), z=dev(z), accum=acc, alpha=0.25, D=D)
        exact(host(acc)[0], bwd_ref.eltwise(7, x, z=z, alpha=0.25, D=D)["accum"],
              bwd_ref.eltwise(7, x, z=z, alpha=0.25, D=D, magnitude=True)["accum"], 4, "eltwise 7", acc0)
    elif mode == 8:
        tab, ids = ints(rng, (997, D), -1, 1), rng.integers(0, 997, rows).astype(np.int32)
        ops.eltwise(8, n, dev(tab), z=dev(ids), accum=acc, alpha=0.5, D=D)
        r = bwd_ref.eltwise(8, tab, z=ids, alpha=0.5, D=D)["accum"]
        exact(host(acc)[0], r, r, 2, "eltwise 8", acc0)


def test_eltwise_real_valued(hip_lib):
    from mvin_amd import ops
    rng = np.random.default_rng(9400)
    rows, D, N = 510, 12, 5          # accumulating modes: rows * D = 6 120 terms (<= 8 192)
    n = rows * D
    x, y, z, zr = reals(rng, n), reals(rng, n), reals(rng, n), reals(rng, rows)
    f32 = lambda v: float(np.float32(v))

    def run(mode, x_, y_=None, z_=None, accum=False, **kw):
        ty = dev(y_) if y_ is not None else None
        acc = torch.zeros(1, dtype=torch.float32, device=DEV) if accum else None
        ops.eltwise(mode, kw.pop("count", n), dev(x_), ty, dev(z_) if z_ is not None else None, accum=acc, **kw)
        return host(acc)[0] if accum else host(ty)

    for mode, args, kw, key, terms in (
            (0, (x, y), dict(alpha=0.3, beta=-1.7), "y", 2), (2, (x, y, z), {}, "y", 1),
            (3, (x,), dict(alpha=0.3), "accum", n), (5, (x, y, zr), dict(alpha=0.3, beta=0.7, D=D), "y", 2),
            (6, (x, np.zeros(n // N, np.float32)), dict(alpha=0.3, D=D, N=N, count=n // N), "y", N),
            (7, (x, None, zr), dict(alpha=0.3, D=D), "accum", n)):
        kwr = {k: (f32(v) if isinstance(v, float) else v) for k, v in kw.items() if k != "count"}
        ref = bwd_ref.eltwise(mode, *args, **kwr)[key]
        mag = bwd_ref.eltwise(mode, *args, magnitude=True, **kwr)[key]
        summed(run(mode, *args, accum=key == "accum", **dict(kw)), ref, mag, terms, f"eltwise {mode} real")
    ids = rng.integers(0, rows, 600).astype(np.int32)
    acc = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.eltwise(8, 600 * D, dev(x), z=dev(ids), accum=acc, alpha=0.3, D=D)
    r = bwd_ref.eltwise(8, x, z=ids, alpha=f32(0.3), D=D)["accum"]
    summed(host(acc)[0], r, r, 600 * D, "eltwise 8 real")
    # 1: sigmoid cross entropy (expf, log1pf, a division) -- the project's tolerance
    s, lab = reals(rng, n, 3.0), (rng.random(n) < 0.5).astype(np.float32)
    ty, acc = torch.zeros(n, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.eltwise(1, n, dev(s), ty, dev(lab), accum=acc, alpha=1.0 / n, beta=1.0 / n)
    ref = bwd_ref.eltwise(1, s, z=lab, alpha=f32(1.0 / n), beta=f32(1.0 / n))
    with bwd_ref.precision(np.float32):
        r32 = bwd_ref.eltwise(1, s, z=lab, alpha=f32(1.0 / n), beta=f32(1.0 / n))
    toleranced(host(ty), ref["y"], r32["y"], "eltwise 1 dscores")
    toleranced(host(acc)[0], ref["accum"], r32["accum"], "eltwise 1 loss")
    # 4: one Adam step
    g, m, v = reals(rng, n), reals(rng, n, 0.1), np.abs(reals(rng, n, 0.1))
    tx, tm, tv = dev(x), dev(m), dev(v)
    hyp = dict(alpha=f32(0.01), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))
    ops.eltwise(4, n, tx, dev(g), tm, tv, **hyp)
    ref = bwd_ref.eltwise(4, x, g, m, v, **hyp)
    with bwd_ref.precision(np.float32):
        r32 = bwd_ref.eltwise(4, x, g, m, v, **hyp)
    for t, k in ((tx, "x"), (tm, "z"), (tv, "w")):
        toleranced(host(t), ref[k], r32[k], f"eltwise 4 {k}")


# ----------------------------------------------------------------------------------------------- L2 + Adam
def _segments(rng, lengths, real, misalign):
    """Parameters laid out in ONE device buffer at float offsets that are deliberately off a 16-byte boundary for some
    segments (``misalign``); returns host arrays, the float offsets and the buffer size."""
    xs, offs, pos = [], [], 0
    for i, n in enumerate(lengths):
        pos = (pos + 3) // 4 * 4 + (misalign[i % len(misalign)])
        offs.append(pos)
        xs.append(reals(rng, n) if real else ints(rng, n, -3, 3))
        pos += n
    return xs, offs, pos + 4


def _seg_table(buf, offs, lengths, l2s):
    table = np.zeros(len(offs), dtype=[("x", "<u8"), ("off", "<i8"), ("n", "<i8"), ("l2", "<f4"), ("pad", "<i4")])
    flat = 0
    for i, (o, n, c) in enumerate(zip(offs, lengths, l2s)):
        table[i] = (buf.data_ptr() + 4 * o, flat, n, c, 0)
        flat += n
    return torch.from_numpy(table.view(np.uint8).copy()).to(DEV), flat


def _lengths(rng, nseg):
    base = [1, 3, 5, 4, 64, 17, 4096 + 2]
    if nseg <= len(base):
        return base[:nseg]
    return base + [int(v) for v in rng.integers(1, 41, nseg - len(base) - 1)] + [70001]


@pytest.mark.parametrize("nseg", [1, 7, 256])
def test_l2_terms_exact_over_a_segment_table(nseg, hip_lib):
    """apply_adam = 0 on integers: g += c x and loss += (c / 2) sum x^2 only; parameters and moments untouched."""
    from mvin_amd import ops
    rng = np.random.default_rng(9500 + nseg)
    lengths = _lengths(rng, nseg)
    l2s = [(0.5, 0.0, 2.0, 0.25)[i % 4] for i in range(nseg)]
    xs, offs, size = _segments(rng, lengths, False, (0, 1, 0, 3, 2))
    hbuf = np.full(size, 77.0, np.float32)
    for x, o in zip(xs, offs):
        hbuf[o:o + x.size] = x
    buf = dev(hbuf)
    segs, total = _seg_table(buf, offs, lengths, l2s)
    g0 = ints(rng, total, -4, 4)
    g, loss = dev(g0), torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    m = torch.full((total,), 11.0, dtype=torch.float32, device=DEV)
    v = torch.full((total,), 13.0, dtype=torch.float32, device=DEV)
    ops.l2_adam_multi(segs, nseg, total, g, m, v, loss, False, 0.1, 0.9, 0.999, 1e-8)
    ref, mag = bwd_ref.l2_adam(xs, l2s, g0), bwd_ref.l2_adam(xs, l2s, g0, magnitude=True)
    exact(host(g), ref["g"], mag["g"], 4, f"l2 nseg={nseg} g")
    exact(host(loss)[0], ref["loss"], mag["loss"], 8, f"l2 nseg={nseg} loss", 3.0)
    np.testing.assert_array_equal(host(buf), hbuf)             # parameters and the gaps between them untouched
    assert torch.all(m == 11.0) and torch.all(v == 13.0)


@pytest.mark.parametrize("nseg,lr_on_device", [(1, False), (7, True), (7, False), (256, True)])
def test_l2_adam_three_steps_real_valued(nseg, lr_on_device, hip_lib):
    """Parameters, m and v after three steps against train_ref.AdamRef in float64 (the L2 gradient added first)."""
    from mvin_amd import ops
    rng = np.random.default_rng(9600 + nseg)
    lengths = _lengths(rng, nseg)
    l2s = [(1e-3, 0.0, 1e-2, 1e-4)[i % 4] for i in range(nseg)]
    xs, offs, size = _segments(rng, lengths, True, (0, 1, 0, 3, 2))
    hbuf = np.zeros(size, np.float32)
    for x, o in zip(xs, offs):
        hbuf[o:o + x.size] = x
    buf = dev(hbuf)
    segs, total = _seg_table(buf, offs, lengths, l2s)
    names = [str(i) for i in range(nseg)]
    # the hyper-parameters as the kernel receives them (floats): float32(0.999) is 1.3e-5 away from 0.999 in 1 - beta2
    lr, (b1, b2, eps) = 0.01, (float(np.float32(h)) for h in (0.9, 0.999, 1e-8))
    opts = {dt: train_ref.AdamRef(dict(zip(names, xs)), lr, b1, b2, eps, dtype=dt) for dt in (np.float64, np.float32)}
    ps = {dt: {k: x.astype(dt) for k, x in zip(names, xs)} for dt in opts}
    m, v = torch.zeros(total, dtype=torch.float32, device=DEV), torch.zeros(total, dtype=torch.float32, device=DEV)
    lr_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    edges = np.cumsum([0] + lengths)
    small = np.zeros(total, bool)
    for t in range(1, 4):
        graw = reals(rng, total)
        graw = np.where(np.abs(graw) < 1e-2, np.copysign(1e-2, graw), graw).astype(np.float32)   # no |g| near zero
        g, loss = dev(graw), torch.zeros(1, dtype=torch.float32, device=DEV)
        lr_t = np.float32(lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t))
        lr_dev.fill_(float(lr_t))
        ops.l2_adam_multi(segs, nseg, total, g, m, v, loss, True, float(lr_t), b1, b2, eps,
                          lr_dev=lr_dev if lr_on_device else None)
        gall, l2l = {}, {}
        for dt, opt in opts.items():      # the same formula in float64 (the reference) and in float32 (its own error)
            grads = {k: graw[edges[i]:edges[i + 1]].astype(dt) + dt(np.float32(l2s[i])) * ps[dt][k]
                     for i, k in enumerate(names)}
            gall[dt] = np.concatenate([grads[k] for k in names])
            l2l[dt] = sum(dt(0.5) * dt(np.float32(l2s[i])) * (ps[dt][k] * ps[dt][k]).sum(dtype=dt) for i, k in enumerate(names))
            ps[dt] = opt.step(ps[dt], grads)
        small |= np.abs(gall[np.float64]) < 1e-6 * np.abs(gall[np.float64]).max()
        toleranced(host(g), gall[np.float64], gall[np.float32], f"adam step {t} g")
        toleranced(host(loss)[0], l2l[np.float64], l2l[np.float32], f"adam step {t} loss")
    assert not small.any(), "case bug: the float64 reference has gradients below 1e-6 max|g|"
    assert small.mean() <= 0.01
    cat = lambda d: np.concatenate([np.asarray(d[k]).ravel() for k in names])
    got_p = np.concatenate([host(buf)[o:o + n] for o, n in zip(offs, lengths)])
    keep = ~small
    toleranced(got_p[keep], cat(ps[np.float64])[keep], cat(ps[np.float32])[keep], "adam parameters after 3 steps")
    toleranced(host(m), cat(opts[np.float64].m), cat(opts[np.float32].m), "adam m after 3 steps")
    toleranced(host(v), cat(opts[np.float64].v), cat(opts[np.float32].v), "adam v after 3 steps")
