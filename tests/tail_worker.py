"""Cases of mvin_l2_tail_fwd for tests/test_gpu_tail.py, and the process that runs them through the other dim-64 kernel.

launch_l2_tail reads MVIN_TAIL_FLASH once per process: unset (the default) every shape takes the tile-image kernel l2_tail_kernel<16 / 32 / 64>
(mvin_tail.hip); with MVIN_TAIL_FLASH=1 dim 64 with an fp32 table and the projection on takes l2_tail_flash_kernel (mvin_tail_flash.hip) and
everything else (dim 16 / 32, a bf16 table, W0 == NULL) still takes the tile-image kernel.  So

    MVIN_TAIL_FLASH=1 python tests/tail_worker.py OUT.pkl

runs every case of CASES (twice each, NaN-filled outputs) and pickles {case name: result dict of numpy arrays}; the test module runs the same
cases in its own process and compares both with float64 and with each other.

A case is a dict of options (``spec``) turned into host arrays by ``Case`` (seeded by the case's name: the same in every process) and run by
``run``.  EXACT cases (real=False) hold small integers: values in [-3, 3], weight blocks with 4 non-zeros in [-2, 2] per column; REAL cases
normal x 0.3 (as tests/test_gpu_fold_f64.py) with at least YARD_ROWS rows, of which the kernels get the first B.  The references
(``reference``, ``magnitude``) are fold_ref.tail_reference over the host arrays: they run without a device too."""
import ctypes
import os
import pickle
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fold_ref                                                                          # noqa: E402
from linear_valu_worker import DEV, dev, ints, poisoned_empty, reals, same_bits, to_bf16      # noqa: E402

F64 = np.float64
DIMS = (16, 32, 64)
# 32-row tiles of the tile-image kernel; 16-pair wave tiles and 192-pair workgroups (12 waves) of the flash kernel
B_LIST = (1, 15, 16, 17, 31, 32, 33, 95, 191, 192, 193, 400)
B_SUBSET = (1, 17, 33, 95, 193, 400)
# a workgroup walks more than one tile -- the only sizes at which the look-ahead loads run:
FLASH_WALK_B = 49152 + 213            # flash: 256 workgroups x 12 waves x 16 pairs per sweep
TILE_WALK_B = 32768 + 33              # tile image, dim 64: 1024 workgroups x 32 rows
TILE_WALK_B_SMALL = 70000             # tile image, dim 16 / 32: 2048 workgroups x 32 rows
LEGACY_B = (1, 15, 16, 17, 33, 500, 4099, 70000)      # the batch sizes of the module's first cases
N_ENTITY = 97
YARD_ROWS = 256
GUARD = 64
DEFAULTS = dict(real=False, i64=True, bias=True, proj=True, uo_is_q=False, bf16=False, null=None, ids=None, nE=N_ENTITY, legacy=None)
# ids outside the table: the entry point reads the WHOLE id as an unsigned 64-bit number (int32 ids sign-extended) and clamps it to n_entity - 1
BAD_IDS64 = (-1, -2 ** 31, -2 ** 32, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 3, 2 ** 63 - 1)
BAD_IDS32 = (-1, -2 ** 31, N_ENTITY, 2 ** 31 - 1)
# the options that are crossed sparsely: they rotate over the batch sizes, shifted per dim, so that every dim meets every one of them
OPTIONS = [("plain", dict()), ("i32", dict(i64=False)), ("nobias", dict(bias=False)), ("noW0", dict(proj=False)), ("uoq", dict(uo_is_q=True)),
           ("bf16", dict(bf16=True)), ("null", dict(null="both")), ("i32_nobias_uoq", dict(i64=False, bias=False, uo_is_q=True)),
           ("noW0_bf16_i32_nobias", dict(proj=False, bf16=True, i64=False, bias=False)), ("nullitem_i32_nobias", dict(null="item", i64=False, bias=False)),
           ("nullsig_uoq", dict(null="sig", uo_is_q=True))]


def flash_applies(spec):
    """l2_tail_flash_applies (mvin_tail_flash.hip) for a process with MVIN_TAIL_FLASH=1."""
    s = dict(DEFAULTS, **spec)
    return s["D"] == 64 and not s["bf16"] and s["proj"]


def sparse_ints(rng, Din, Dout, nnz=4):
    """[Din, Dout] with nnz non-zeros out of {-2, -1, 1, 2} per column."""
    W = np.zeros((Din, Dout), np.float32)
    for j in range(Dout):
        W[rng.choice(Din, min(nnz, Din), replace=False), j] = rng.choice([-2, -1, 1, 2], min(nnz, Din))
    return W


def _family(real, Bs_by_dim):
    fam = "real" if real else "exact"
    cases = {}
    for di, D in enumerate(DIMS):
        for B in Bs_by_dim[D]:
            bi = B_LIST.index(B)
            tag, opt = OPTIONS[(bi + 5 * di + (3 if real else 0)) % len(OPTIONS)]
            spec = dict(opt, D=D, B=B, real=real)
            cases[f"{fam}_D{D}_B{B}_{tag}"] = spec
            if D == 64 and not flash_applies(spec):       # every batch size through the flash kernel too
                cases[f"{fam}_D{D}_B{B}_flash{bi % 4}"] = dict(D=D, B=B, real=real, i64=bi % 2 == 0, bias=bi % 4 < 2)
    return cases


def build_cases():
    cases = _family(False, {D: B_LIST for D in DIMS})
    cases.update(_family(True, {16: B_SUBSET, 32: B_SUBSET, 64: B_LIST}))
    cases[f"real_D64_B{FLASH_WALK_B}_walk"] = dict(D=64, B=FLASH_WALK_B, real=True)
    cases[f"real_D64_B{TILE_WALK_B}_walk"] = dict(D=64, B=TILE_WALK_B, real=True)
    cases[f"real_D32_B{TILE_WALK_B_SMALL}_walk"] = dict(D=32, B=TILE_WALK_B_SMALL, real=True)
    cases[f"real_D16_B{TILE_WALK_B_SMALL}_walk"] = dict(D=16, B=TILE_WALK_B_SMALL, real=True)
    for D, opt in ((64, dict()), (64, dict(proj=False)), (64, dict(bf16=True)), (32, dict()), (16, dict())):
        tag = "".join("_" + k for k in opt)
        cases[f"ids_D{D}{tag}_i64"] = dict(opt, D=D, B=100, real=True, ids="bad")
        cases[f"ids_D{D}{tag}_i32"] = dict(opt, D=D, B=100, real=True, ids="bad", i64=False)
    # the inputs of test_tail_against_float64 at dim 64 (uniform(-0.5, 0.5), 3000 entities) and of the kernel-against-kernel test
    for B, i64 in [(B, True) for B in LEGACY_B] + [(17, False), (4099, False)]:
        cases[f"legacy_D64_B{B}_{'i64' if i64 else 'i32'}"] = dict(D=64, B=B, real=True, i64=i64, nE=3000, legacy=64 + B)
    cases["legacy_D64_B5000_seed11"] = dict(D=64, B=5000, real=True, nE=3000, legacy=11)
    return cases


def legacy_inputs(B, D, n_entity, seed, idt=torch.int64):
    """Device tensors of the module's first cases: uniform(-0.5, 0.5), weights scaled by 0.3 - 0.4 (drawn on the device: the same in every process)."""
    dv = torch.device(DEV)
    g = torch.Generator(device=dv)
    g.manual_seed(seed)
    rnd = lambda *s: torch.rand(s, device=dv, generator=g) - 0.5      # noqa: E731
    E = rnd(n_entity, D)
    items = torch.randint(0, n_entity, (B,), device=dv, generator=g).to(idt)
    q, uo, n0, n1 = rnd(B, D), rnd(B, D), rnd(B, D), rnd(B, D)
    W0, A0, A1, Wmix = rnd(D, D) * 0.4, rnd(D, D) * 0.4, rnd(D, D) * 0.4, rnd(3 * D, D) * 0.3
    b0, a0, a1, bmix = rnd(D), rnd(D), rnd(D), rnd(D)
    return E, items, q, uo, n0, n1, W0, b0, A0, a0, A1, a1, Wmix, bmix


def clamp_tail_ids(items, n_entity):
    """Item ids as mvin_l2_tail_fwd reads them: whole, as unsigned 64-bit numbers (int32 sign-extended), clamped to the table's last row."""
    u = np.asarray(items).astype(np.int64).view(np.uint64)
    return np.minimum(u, np.uint64(n_entity - 1)).astype(np.int64)


class Case(object):
    def __init__(self, name, spec):
        s = dict(DEFAULTS, **spec)
        self.name, self.spec = name, s
        assert s["legacy"] is None, "legacy cases are drawn on the device (legacy_inputs)"
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        D, B, real, nE = s["D"], s["B"], s["real"], s["nE"]
        self.D, self.B, self.nE = D, B, nE
        self.n = n = max(B, YARD_ROWS) if real else B
        val = (lambda shape: reals(rng, shape, 0.3)) if real else (lambda shape: ints(rng, shape, -3, 3))
        wgt = (lambda a, b: reals(rng, (a, b), 0.3)) if real else (lambda a, b: sparse_ints(rng, a, b))
        E = val((nE, D))
        self.E = to_bf16(E) if s["bf16"] else E
        idt = np.int64 if s["i64"] else np.int32
        self.items = rng.integers(0, nE, n).astype(idt)
        self.bad_at = None
        if s["ids"] == "bad":
            bad = BAD_IDS64 if s["i64"] else BAD_IDS32
            self.bad_at = 3 + 7 * np.arange(2 * len(bad))            # rows of several wave tiles and of all four 32-row tiles
            assert self.bad_at.max() < B
            self.items[self.bad_at] = np.array(bad * 2, dtype=idt)
        self.q, self.n0, self.n1 = val((n, D)), val((n, D)), val((n, D))
        self.uo = self.q if s["uo_is_q"] else val((n, D))
        self.W0 = wgt(D, D) if s["proj"] else None
        self.A0, self.A1 = wgt(D, D), wgt(D, D)
        self.Wmix = np.concatenate([wgt(D, D) for _ in range(3)], axis=0)
        self.b0, self.a0, self.a1, self.bmix = (val((D,)) if s["bias"] else None for _ in range(4))
        if not s["proj"]:
            self.b0 = None

    def host_args(self, absolute=False):
        """The arguments of fold_ref.tail_reference after (E, x) as float32 host arrays (their absolute values: the magnitudes)."""
        a = (self.q, self.uo, self.n0, self.n1, self.W0, self.b0, self.A0, self.a0, self.A1, self.a1, self.Wmix, self.bmix)
        return [None if t is None else (np.abs(t) if absolute else t) for t in a]


def reference(case, dtype=torch.float64, device="cpu", absolute=False):
    """fold_ref.tail_reference over all rows of the case -> (item_emb, scores, sigmoid) tensors of ``dtype`` on ``device``.  ``absolute``: the
    same sums over the absolute values of every input in float64 -- a bound of every partial sum of every evaluation order (ReLU only shrinks)."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    x = t(clamp_tail_ids(case.items, case.nE))
    E = np.abs(case.E) if absolute else case.E
    q = t(case.host_args(absolute)[0]) if case.W0 is not None else None
    return fold_ref.tail_reference(t(E), x, q, *[t(a) for a in case.host_args(absolute)[1:]], dtype=dtype)


def magnitude(case, device="cpu"):
    return reference(case, torch.float64, device, absolute=True)


def exact(got, ref, mag, denom, what):
    """got == ref exactly, after checking on the reference that float32 holds every partial sum (tests/test_gpu_fwd_kernels.py)."""
    ref, mag = np.asarray(ref, F64), np.asarray(mag, F64)
    assert np.all(mag * denom < 2.0 ** 24), f"{what}: case bug: sum|terms| * {denom} = {mag.max() * denom:.4g} >= 2^24"
    assert np.all(np.abs(ref) <= mag), f"{what}: case bug: magnitude below the value"
    assert np.array_equal(ref * denom, np.round(ref * denom)), f"{what}: case bug: reference is not a multiple of 1/{denom}"
    np.testing.assert_array_equal(np.asarray(got, F64).reshape(ref.shape), ref, err_msg=what)


# ----------------------------------------------------------------------------------------------- run
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _twice(launch, what):
    first = None
    for _ in range(2):
        got = launch()
        torch.cuda.synchronize()
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert (a is None) == (b is None) and (a is None or same_bits(a, b)), f"{what}: two launches differ"
    return first


def _np(t):
    return None if t is None else t.cpu().numpy()


def _through_ops(args, what):
    from mvin_amd import ops

    def launch():
        with poisoned_empty():
            return ops.l2_tail(*args)

    item, scores, sig = _twice(launch, what)
    return {"item_emb": _np(item), "scores": _np(scores), "sigmoid": _np(sig)}


def _direct(args, null, bf16, what):
    """hip_lib.mvin_l2_tail_fwd itself with item_emb and / or sig NULL: every output buffer NaN with a guard tail; the omitted buffers are
    not passed and, like the guards, must stay NaN."""
    from mvin_amd import _lib
    lib = _lib.load()
    E, items, q, uo, n0, n1, W0, b0, A0, a0, A1, a1, Wmix, bmix = args
    B, D = uo.shape
    i64, i32 = (items, None) if items.dtype == torch.int64 else (None, items)

    def launch():
        nan = lambda n: torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)      # noqa: E731
        item, scores, sig = nan(B * D), nan(B), nan(B)
        rc = lib.mvin_l2_tail_fwd(_ptr(E), _ptr(i64), _ptr(i32), _ptr(q), _ptr(uo), _ptr(n0), _ptr(n1), _ptr(W0), _ptr(b0), _ptr(A0), _ptr(a0),
                                  _ptr(A1), _ptr(a1), _ptr(Wmix), _ptr(bmix), B, D, E.shape[0], None if null in ("both", "item") else _ptr(item),
                                  _ptr(scores), None if null in ("both", "sig") else _ptr(sig), 1 if bf16 else 0,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, f"{what}: mvin_l2_tail_fwd returned {rc}"
        return item, scores, sig

    item, scores, sig = _twice(launch, what)
    res = {"guards_nan": bool(torch.isnan(item[B * D:]).all() and torch.isnan(scores[B:]).all() and torch.isnan(sig[B:]).all()),
           "omitted_nan": bool((null == "sig" or torch.isnan(item).all()) and (null == "item" or torch.isnan(sig).all())),
           "item_emb": None if null in ("both", "item") else _np(item[: B * D].view(B, D)), "scores": _np(scores[:B]),
           "sigmoid": None if null in ("both", "sig") else _np(sig[:B])}
    return res


def device_args(case, items=None):
    s, B = case.spec, case.B
    q = dev(case.q[:B])
    uo = q if s["uo_is_q"] else dev(case.uo[:B])
    o = lambda a: None if a is None else dev(a)      # noqa: E731
    return (dev(case.E, s["bf16"]), dev(case.items[:B] if items is None else items), q if s["proj"] else None, uo, dev(case.n0[:B]),
            dev(case.n1[:B]), o(case.W0), o(case.b0), o(case.A0), o(case.a0), o(case.A1), o(case.a1), o(case.Wmix), o(case.bmix))


def run(name, spec):
    """-> result dict: item_emb [B, D] / scores [B] / sigmoid [B] as float32 numpy arrays (None where the case omits the output), the flags of
    the direct calls, and for the id cases ``clamped``: the result of the same call with the ids clamped on the host."""
    s = dict(DEFAULTS, **spec)
    if s["legacy"] is not None:
        return _through_ops(legacy_inputs(s["B"], s["D"], s["nE"], s["legacy"], torch.int64 if s["i64"] else torch.int32), name)
    case = Case(name, spec)
    if s["null"]:
        return _direct(device_args(case), s["null"], s["bf16"], name)
    res = _through_ops(device_args(case), name)
    if s["ids"]:
        clamped = clamp_tail_ids(case.items[: case.B], case.nE).astype(case.items.dtype)
        assert (clamped[case.bad_at] == case.nE - 1).all() and int((clamped != case.items[: case.B]).sum()) == len(case.bad_at)
        res["clamped"] = _through_ops(device_args(case, clamped), name + " (ids clamped on the host)")
    return res


CASES = build_cases()

if __name__ == "__main__":
    assert os.environ.get("MVIN_TAIL_FLASH") == "1", "this process exists to run the dim-64 cases through l2_tail_flash_kernel"
    with open(sys.argv[1], "wb") as f:
        pickle.dump({name: run(name, spec) for name, spec in CASES.items()}, f, protocol=4)
