"""Cases of mvin_linear_fwd for tests/test_gpu_fwd_kernels.py, and the process that runs the matrix-core shapes through the
other kernel.

launch_linear reads MVIN_LINEAR_VALU once per process: with it set, linear_kernel<NR> (mvin_kernels.hip) takes the 14 shapes
linear_mfma_kernel<D, NE> (mvin_linear_mfma.hip) takes by default.  So

    MVIN_LINEAR_VALU=1 python tests/linear_valu_worker.py OUT.pkl

runs every case of MFMA_CASES (twice each, NaN-filled buffers) and pickles {case name: result dict of numpy arrays}; the test
module runs the same cases in its own process and compares both with float64 and with each other.

A case is a dict of options (``spec``) turned into host arrays by ``build`` (seeded by the case's name: the same in every
process), run by ``run``.  EXACT cases (real=False) hold small integers: values in [-3, 3], weights in [-2, 2]."""
import contextlib
import os
import pickle
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
ROWS = (1, 17, 32, 33, 95)
MFMA_SHAPES = [(D, ne) for D in (16, 32, 64) for ne in (1, 2, 3, 4)] + [(128, 1), (128, 2)]      # (Dout, Din / Dout)
DEFAULTS = dict(sum=False, gather=None, bf16=False, identity=False, bias=False, rowbias=None, relu=False, off=0, pad=0, nz=1,
                zs=False, score=False, real=False, ntab=7, bad_ids=False)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def reals(rng, shape, scale=1.0):
    """Gaussians with |x| >= 2^-10 * scale: products of two of them are far from subnormal."""
    a = rng.standard_normal(shape)
    a = np.where(np.abs(a) < 2.0 ** -10, np.copysign(2.0 ** -10, a), a)
    return (a * scale).astype(np.float32)


def to_bf16(a):
    """The float32 values a bf16 table holds."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(torch.bfloat16) if bf16 else t


@contextlib.contextmanager
def poisoned_empty():
    """Every buffer an ops wrapper allocates with torch.empty starts as NaN (integers: -7777), so an element a kernel leaves
    unwritten cannot look right by accident."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-7777)

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------- the case list
def plain_path(Din):
    """linear_mfma_kernel stages one contiguous fp32 source of full width with every load of the tile in flight only when the
    32 x Din / 4 chunks of a tile are a whole number of rounds of the 256 threads: Din % 32 == 0."""
    return (32 * Din // 4) % 256 == 0


def staging_forms(width, ne):
    """(tag, options) of the ways a [rows, ne * width] input is staged."""
    Din = ne * width
    forms = [("plain", dict(nsrc=1, Dsrc=Din))]
    if ne > 1:
        forms.append(("concat", dict(nsrc=ne, Dsrc=width)))
    mixed = ["i32" if s != 1 else None for s in range(ne)]             # source 1 (if any) stays dense beside gathered ones
    forms += [("gather32", dict(nsrc=ne, Dsrc=width, gather=mixed)), ("gather64", dict(nsrc=ne, Dsrc=width, gather=["i64"] * ne)),
              ("bf16", dict(nsrc=ne, Dsrc=width, bf16=True, gather=(["i32"] * ne if ne % 2 else None))),
              ("sum2", dict(nsrc=2, Dsrc=Din, sum=True)), ("sum3", dict(nsrc=3, Dsrc=Din, sum=True, gather=["i32", None, "i32"]))]
    return forms


def option_sets(rows):
    return [("bias_relu", dict(bias=True, relu=True)), ("rowbias1", dict(rowbias=1)), ("rowbias3", dict(rowbias=3, bias=True)),
            ("rowbiasR", dict(rowbias=rows, relu=True)), ("window", dict(off=3, pad=5, bias=True)),
            ("score", dict(score=True)), ("score_all", dict(score=True, bias=True, rowbias=3, relu=True, off=1, pad=2))]


def shape_cases(Dout, ne, width=None, walk=True):
    """Every case of one shape, Din = ne * width (width = Dout: a matrix-core shape): staging forms x row counts, the options,
    the z-batched launches."""
    width = width or Dout
    cases, Din, p = {}, ne * width, f"D{Dout}_{ne}x{width}"
    for fi, (tag, form) in enumerate(staging_forms(width, ne)):
        for ri, rows in enumerate(ROWS):
            cases[f"{p}_{tag}_r{rows}_exact"] = dict(form, Dout=Dout, rows=rows)
            if (fi + ri) % 2 == 0 or rows == 95:
                cases[f"{p}_{tag}_r{rows}_real"] = dict(form, Dout=Dout, rows=rows, real=True)
    base = dict(nsrc=ne, Dsrc=width, Dout=Dout) if ne > 1 else dict(nsrc=1, Dsrc=Din, Dout=Dout)
    for rows in (33, 95):
        for tag, opt in option_sets(rows):
            if opt.get("score") and Dout > Din + 4:
                continue                # the entry point refuses it
            for real in (False, True):
                cases[f"{p}_{tag}_r{rows}_{'real' if real else 'exact'}"] = dict(base, rows=rows, real=real, **opt)
    if walk:
        # more tiles than workgroups: linear_mfma_kernel's grid is ceil(256 CUs * (12 | 4) / nz) = 1 workgroup per z, which
        # walks the 3 tiles of 70 rows
        nz = 3072 if ne == 1 else 1024
        cases[f"{p}_walk_z{nz}_exact"] = dict(base, rows=70, nz=nz, bias=True, relu=True)
        cases[f"{p}_walk_z{nz}_real"] = dict(base, rows=70, nz=nz, bias=True, real=True)
    for real in (False, True):
        cases[f"{p}_zstrides_{'real' if real else 'exact'}"] = dict(base, rows=37, nz=3, zs=True, bias=True, pad=3, off=2, real=real)
    return cases


MFMA_CASES = {}
for _D, _ne in MFMA_SHAPES:
    MFMA_CASES.update(shape_cases(_D, _ne))


# ----------------------------------------------------------------------------------------------- build / run
class Case(object):
    def __init__(self, name, spec):
        s = dict(DEFAULTS, **spec)
        self.name, self.spec = name, s
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        nsrc, Dsrc, Dout, rows, real = s["nsrc"], s["Dsrc"], s["Dout"], s["rows"], s["real"]
        self.Din = Din = Dsrc if s["sum"] else nsrc * Dsrc
        val = (lambda shape: reals(rng, shape)) if real else (lambda shape: ints(rng, shape, -3, 3))
        wgt = (lambda shape: reals(rng, shape)) if real else (lambda shape: ints(rng, shape, -2, 2))
        gather = s["gather"] or [None] * nsrc
        self.ids64 = any(g == "i64" for g in gather)
        self.srcs, self.ids = [], []
        for g in gather:
            a = val((s["ntab"] if g else rows + 2, Dsrc))
            self.srcs.append(to_bf16(a) if s["bf16"] else a)
            self.ids.append(rng.integers(0, s["ntab"], rows).astype(np.int64 if self.ids64 else np.int32) if g else None)
        self.src_rows = s["ntab"] if any(gather) else 0
        if s["bad_ids"]:
            # outside [0, ntab): past the end, negative, the extremes of the id type
            bad = [s["ntab"], -1, s["ntab"] + 5, -2 ** 31, 2 ** 31 - 1] + ([2 ** 40, -2 ** 40, -2 ** 63, 2 ** 63 - 1] if self.ids64 else [])
            for i in self.ids:
                if i is not None:
                    n = min(len(bad), rows)
                    i[rng.choice(rows, n, replace=False)] = bad[:n]
        self.nz = nz = s["nz"]
        self.ldo = Dout + s["pad"]
        self.wzs, self.bzs, self.ozs = (Din * Dout + 8, Dout + 4, rows * self.ldo + 12) if s["zs"] else (0, 0, rows * self.ldo)
        self.W = None if s["identity"] else wgt((nz - 1) * self.wzs + Din * Dout)
        self.bias = wgt((nz - 1) * self.bzs + Dout) if s["bias"] else None
        self.rpg = s["rowbias"] or 1
        self.rowbias = wgt(((rows + self.rpg - 1) // self.rpg, Dout)) if s["rowbias"] else None
        # score_u of a real-valued case is scaled so that the score is of order 1 and the sigmoid is not saturated
        self.score_u = (val((rows, Dout)) * (np.float32(1.0 / np.sqrt(Din * Dout)) if real else np.float32(1))) if s["score"] else None
        self.off = s["off"]
        self.out_elems = self.off + (nz - 1) * self.ozs + rows * self.ldo + 7
        self.walk = nz > 16           # the z-batched walk cases: every slab the same; slab 0 is kept

    def ref_kwargs(self):
        """Keyword arguments of fwd_ref.linear (out: a compact [nz, rows, Dout]); the walk cases as their slab 0."""
        s = self.spec
        return dict(srcs=self.srcs, W=self.W, Dout=s["Dout"], rows=s["rows"], ids=self.ids, bias=self.bias, rowbias=self.rowbias,
                    rows_per_group=self.rpg, relu=s["relu"], sum_sources=s["sum"], nz=1 if self.walk else self.nz,
                    w_zstride=self.wzs, bias_zstride=self.bzs, src_rows=self.src_rows, score_u=self.score_u)

    def terms(self):
        """Number of terms of one output element, bias and row bias counted."""
        s = self.spec
        n = s["nsrc"] if s["identity"] else (s["nsrc"] * s["Dsrc"] if s["sum"] else self.Din)
        return n + (self.bias is not None) + (self.rowbias is not None)


def run(case):
    """Two launches into NaN-filled buffers, equal bits -> dict(out [nz, rows, Dout], clean: nothing else of the buffer was
    written, score, sigmoid) as numpy arrays (float32)."""
    from mvin_amd import ops
    s = case.spec
    rows, Dout, nz = s["rows"], s["Dout"], case.nz
    srcs = [dev(a, s["bf16"]) for a in case.srcs]
    ids = [None if i is None else dev(i) for i in case.ids]
    W, bias, rowbias, u = (None if a is None else dev(a) for a in (case.W, case.bias, case.rowbias, case.score_u))
    first = None
    for _ in range(2):
        buf = torch.full((case.out_elems,), float("nan"), dtype=torch.float32, device=DEV)
        with poisoned_empty():
            r = ops.linear(srcs, W, Dout, ids=ids if any(i is not None for i in ids) else None, bias=bias, rowbias=rowbias,
                           rows_per_group=case.rpg, relu=s["relu"], rows=rows, out=buf, out_offset=case.off, ldo=case.ldo, nz=nz,
                           w_zstride=case.wzs, bias_zstride=case.bzs, out_zstride=case.ozs, score_u=u, sum_sources=s["sum"])
        torch.cuda.synchronize()
        got = (buf,) + (tuple(r[1:]) if u is not None else ())
        if first is None:
            first = got
        assert all(same_bits(a, b) for a, b in zip(first, got)), f"{case.name}: two launches differ"
    buf = first[0]
    idx = (case.off + torch.arange(nz, device=DEV)[:, None, None] * case.ozs + torch.arange(rows, device=DEV)[None, :, None] * case.ldo
           + torch.arange(Dout, device=DEV)[None, None, :])
    out = buf[idx]
    rest = buf.clone()
    rest[idx.reshape(-1)] = float("nan")
    res = {"clean": bool(torch.isnan(rest).all()), "score": None, "sigmoid": None}
    if case.walk:
        res["slabs_equal"] = bool(same_bits(out, out[:1].expand_as(out)))
        out = out[:1]
    res["out"] = out.cpu().numpy()
    if u is not None:
        res["score"], res["sigmoid"] = first[1].cpu().numpy(), first[2].cpu().numpy()
    return res


if __name__ == "__main__":
    assert os.environ.get("MVIN_LINEAR_VALU"), "this process exists to run the matrix-core shapes through linear_kernel<NR>"
    with open(sys.argv[1], "wb") as f:
        pickle.dump({name: run(Case(name, spec)) for name, spec in MFMA_CASES.items()}, f)
