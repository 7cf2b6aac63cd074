"""-m gpu: mvin_l2_tail_fwd -- level-0 projection, both hop-0 aggregators, the mix-hop combiner and the score of a depth-2 tree
(model.py:270-317, aggregators.py:108-116, model.py:158-159) -- directly against a float64 evaluation of those formulas, in BOTH of its
kernels.  This process runs the default, the tile-image kernel l2_tail_kernel<16 / 32 / 64> (mvin_tail.hip); ONE child process with
MVIN_TAIL_FLASH=1 (read once per process; tests/tail_worker.py) runs the same case list through l2_tail_flash_kernel (mvin_tail_flash.hip)
where that kernel applies -- dim 64, fp32 table, projection on -- and through the tile-image kernel elsewhere.  Every test of the module
depends on the child's results: a child that ends by signal, abort or timeout fails the fixture and nothing else here launches.

Every launch runs twice with equal bits into NaN-filled outputs (torch.empty is made to fill with NaN for the call; the direct calls
use NaN buffers with a guard tail).

EXACT cases (no tolerance).  Small integers: values in [-3, 3], weight blocks with 4 non-zeros in [-2, 2] per column.  ``exact()`` asserts
on the reference that the sum of |terms| of every output stays below 2^24 (dim 64: item 1.2e4, score 9.4e5) before it compares; then
item_emb and scores equal float64 bit for bit in both processes, the child equals the parent, and the sigmoid lies within 2^-22 of the
float64 sigmoid of the exact score.  D in {16, 32, 64} x B in {1, 15, 16, 17, 31, 32, 33, 95, 191, 192, 193, 400}; int32 / int64 ids, no
biases, W0 = None (ev0 = E[item]), q being user_o itself, a bf16 table, item_emb and / or sig NULL (through the entry point itself; the
omitted buffers and the guards stay NaN) rotate over them, and at dim 64 every B also runs in a form the flash kernel takes.

REAL cases.  Inputs normal x 0.3; per output err_hip = max |kernel - float64| <= 4 err_f32 + 2e-6, err_f32 = max |fp32 evaluation of the
same reference - float64| over at least 256 rows of which the case's are the first (fold_ref.compare; never the kernel).  The B list at
dim 64, {1, 17, 33, 95, 193, 400} at dim 16 / 32, and the sizes at which a workgroup walks more than one tile (the look-ahead loads run
only there): B = 49152 + 213 (flash), 32768 + 33 (tile image, dim 64), 70000 (dim 16 / 32).  The module's first cases (uniform(-0.5, 0.5),
3000 entities, B up to 70000) keep their absolute bounds -- item rtol 1e-5 / atol 2e-6, scores 1e-5 / 4e-6, sigmoid 1e-5 / 1e-6 -- and at
dim 64 hold the child's results to them too.

Dispatch.  The child's REAL results differ in bits from the parent's somewhere over the dim-64 / fp32 / W0 cases (that is how the module
knows the child ran the flash kernel), and equal them bit for bit at dim 16 / 32, with a bf16 table and with W0 = None.

Ids.  An id is read whole, as an unsigned 64-bit number (int32 sign-extended), and clamped to n_entity - 1 (include/mvin_hip.h): int64
{-1, -2^31, -2^32, 2^31, 2^32 + 5, 2^40 + 3, 2^63 - 1} and int32 {-1, INT32_MIN, n_entity, INT32_MAX} give the bits of the same call with
the ids clamped on the host, in both processes.

MEASURED on an MI355X, worst over the REAL cases (err_hip | err_f32 | err_hip / (4 err_f32 + 2e-6); -s prints the lines of a run):
    kernel            item_emb                    scores                      sigmoid
    tile<16>          1.7e-6 | 1.8e-6 | 0.21      2.1e-6 | 1.9e-6 | 0.23      3.2e-7 | 2.9e-7 | 0.10
    tile<32>          6.3e-6 | 7.8e-6 | 0.22      6.9e-6 | 6.6e-6 | 0.24     1.2e-6 | 1.4e-6 | 0.16
    tile<64>          2.1e-5 | 2.3e-5 | 0.31      3.0e-5 | 3.5e-5 | 0.27      4.9e-6 | 8.2e-6 | 0.27
    flash             2.4e-5 | 2.3e-5 | 0.32      3.4e-5 | 3.5e-5 | 0.30      5.4e-6 | 8.2e-6 | 0.28
(the child's tile-image results have the parent's bits, so its figures).  39 exact cases, all bit-equal to float64 in both processes
and between them; exact-case sigmoid at most 0.23 x 2^-22.  The child's bits differed from the parent's in 14 of the 14 real-valued
dim-64 / fp32 / W0 cases and equalled them in all 52 cases the flash kernel declines.  73 tests (18 of them the old skips), 27 s as a
module on its own, of which 23 s are the fixture (opening the device, the child process); the longest test body 0.5 s.

Ids before the fix of l2_tail_flash_kernel (it read the low 32-bit word): ids_D64_i64 failed in the child for -2^32, 2^32 + 5 and
2^40 + 3 (entity 0 / 5 / 3 instead of the last row); every other id case and the parent passed.

That the module bites was checked on a scratch copy of the library with value-only mutations (every address stays in bounds):
  * l2_tail_kernel<D>: a1 taken from a0 -- in the parent all 55 cases of the list with biases fail (15 / 14 / 26 at dim 16 / 32 / 64,
    the id cases by their value check), the same ones in the child where it runs this kernel, and all 30 of
    test_tail_against_float64; the 25 cases without biases, where the mutant computes the same, pass.
  * l2_tail_flash_kernel without the ReLU after the A1 product -- all 28 cases the child runs through it fail (exact ones bitwise, and
    against the parent), all ten dim-64 cases of test_tail_against_float64 and the kernel-against-kernel test.
No other case failed under either.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import fold_ref
import tail_worker as tw
from parity import assert_close
from tail_worker import DEV, legacy_inputs as _inputs

pytestmark = pytest.mark.gpu

NAMES = ("item_emb", "scores", "sigmoid")
STATS = {}
_PARENT, _REFS = {}, {}


def _reference(E, items, q, uo, n0, n1, W0, b0, A0, a0, A1, a1, Wmix, bmix):
    d = lambda t: t.double()      # noqa: E731
    ev0 = (d(E)[items.long()] + d(q)) @ d(W0) + d(b0)
    out0 = torch.relu((ev0 + d(n0)) @ d(A0) + d(a0))
    out2 = torch.relu((out0 + d(n1)) @ d(A1) + d(a1))
    item = torch.cat([ev0, out0, out2], dim=1) @ d(Wmix) + d(bmix)
    s = (d(uo) * item).sum(1)
    return item, s, torch.sigmoid(s)


@pytest.fixture(scope="module")
def flash_results(hip_lib, tmp_path_factory):
    """Every case of tail_worker.CASES in a process with MVIN_TAIL_FLASH=1: one child, once."""
    assert "MVIN_TAIL_FLASH" not in os.environ, "the parent runs the tile-image kernels"
    path = str(tmp_path_factory.mktemp("tail_flash") / "flash.pkl")
    p = subprocess.run([sys.executable, tw.__file__, path], env=dict(os.environ, MVIN_TAIL_FLASH="1"), stdin=subprocess.DEVNULL,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-4000:]}"
    with open(path, "rb") as f:
        return pickle.load(f)


def parent_result(name):
    if name not in _PARENT:
        _PARENT[name] = tw.run(name, tw.CASES[name])
    return _PARENT[name]


def references(name):
    """-> (case, float64 reference, fp32 reference, err_f32 per output over all rows, magnitudes) on the device, computed once."""
    if name not in _REFS:
        case = tw.Case(name, tw.CASES[name])
        r64, r32 = tw.reference(case, torch.float64, DEV), tw.reference(case, torch.float32, DEV)
        yard = [float((b.double() - a).abs().max()) for a, b in zip(r64, r32)]
        _REFS[name] = (case, r64, r32, yard, None if case.spec["real"] else tw.magnitude(case, DEV))
    return _REFS[name]


def kernel_of(name, child):
    D = tw.CASES[name]["D"]
    return "flash" if child and tw.flash_applies(tw.CASES[name]) else f"tile<{D}>" + (" (child)" if child else "")


def check(name, res, child, fails):
    """One result against float64: exact cases bit for bit, real ones by the rule.  Misses go to ``fails``."""
    case, r64, r32, yard, mag = references(name)
    s, B, kernel = case.spec, case.B, kernel_of(name, child)
    what = f"{name} [{kernel}]"
    present = [i for i, n in enumerate(NAMES) if res[n] is not None]
    assert ("item_emb" in [NAMES[i] for i in present]) == (s["null"] not in ("both", "item")) and res["scores"] is not None
    if s["null"]:
        if not (res["guards_nan"] and res["omitted_nan"]):
            fails.append(f"{what}: guard tails NaN: {res['guards_nan']}, omitted outputs NaN: {res['omitted_nan']}")
    for n in NAMES:
        if res[n] is not None and not np.isfinite(res[n]).all():
            fails.append(f"{what} {n}: {int((~np.isfinite(res[n])).sum())} elements left unwritten (or not finite)")
            return
    if s["real"]:
        pick = lambda t: [t[i][:B] for i in present]      # noqa: E731
        got = [torch.from_numpy(res[NAMES[i]]).to(DEV) for i in present]
        fold_ref.compare([NAMES[i] for i in present], got, pick(r64), pick(r32), what, fails, hold_tail=False, stats=STATS, key=kernel,
                         yard=[yard[i] for i in present])
        return
    try:
        for i in [i for i in present if NAMES[i] != "sigmoid"]:
            tw.exact(res[NAMES[i]], r64[i].cpu().numpy(), mag[i].cpu().numpy(), 1, f"{what} {NAMES[i]}")
        if res["sigmoid"] is not None:
            err = float(np.abs(res["sigmoid"].astype(np.float64) - r64[2].cpu().numpy()).max())
            k = (kernel, "exact sigmoid / 2^-22")
            STATS[k] = max(STATS.get(k, 0.0), err / 2.0 ** -22)
            assert err <= 2.0 ** -22, f"{what}: sigmoid {err:.3e} from the float64 sigmoid of the exact score"
    except AssertionError as e:
        fails.append(str(e).strip().splitlines()[0] + " | " + " ".join(str(e).split())[:300])


def report():
    """The worst figures per kernel and output since the last report (one test's)."""
    for key in sorted(STATS):
        v = STATS.pop(key)
        if isinstance(v, list):
            print(f"MEASURED {key[0]} {key[1]}: err_hip {v[0]:.3e} err_f32 {v[1]:.3e} err/(4 err_f32 + 2e-6) {v[2]:.3f}")
        else:
            print(f"MEASURED {key[0]} {key[1]}: {v:.3f}")


def same(a, b):
    return all((a[n] is None) == (b[n] is None) and (a[n] is None or np.array_equal(a[n].view(np.int32), b[n].view(np.int32))) for n in NAMES)


def names_of(family, D=None):
    return [n for n, s in tw.CASES.items() if n.startswith(family + "_") and (D is None or s["D"] == D)]


# ----------------------------------------------------------------------------------------------- the module's first cases
@pytest.mark.parametrize("idt", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 500, 4099, 70000])
@pytest.mark.parametrize("D", [64, 32, 16])
def test_tail_against_float64(D, B, idt, hip_lib, flash_results):
    from mvin_amd import ops
    if idt == torch.int32 and B not in (17, 4099):
        pytest.skip("int32 ids: two sizes")
    assert tuple(tw.LEGACY_B) == (1, 15, 16, 17, 33, 500, 4099, 70000)
    args = _inputs(B, D, 3000, seed=D + B, idt=idt)
    with tw.poisoned_empty():
        item, s, sg = ops.l2_tail(*args)
        again = ops.l2_tail(*args)
    torch.cuda.synchronize()
    assert torch.equal(item, again[0]) and torch.equal(s, again[1])
    ri, rs, rg = (t.cpu().numpy() for t in _reference(*args))
    results = [("tile image", item.cpu().numpy(), s.cpu().numpy(), sg.cpu().numpy())]
    if D == 64:
        c = flash_results[f"legacy_D64_B{B}_{'i64' if idt == torch.int64 else 'i32'}"]
        results.append(("flash (child)", c["item_emb"], c["scores"], c["sigmoid"]))
    for kernel, gi, gs, gg in results:
        assert_close(gi, ri, f"{kernel}: item embeddings vs float64", rtol=1e-5, atol=2e-6)
        assert_close(gs, rs, f"{kernel}: scores vs float64", rtol=1e-5, atol=4e-6)
        assert_close(gg, rg, f"{kernel}: sigmoid scores vs float64", rtol=1e-5, atol=1e-6)


def test_out_of_range_item_id_is_clamped(hip_lib, flash_results):
    from mvin_amd import ops
    args = list(_inputs(100, 64, 500, seed=3))
    bad = args[1].clone()
    bad[::9] = 500 + 77
    args[1][::9] = 499
    x = ops.l2_tail(*args)
    args[1] = bad
    y = ops.l2_tail(*args)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_flash_kernel_agrees_with_the_tile_image_kernel_at_dim_64(hip_lib, flash_results):
    """The same 5000 pairs through l2_tail_flash_kernel (the child) and l2_tail_kernel<64> (this process), each against float64 and
    against each other."""
    from mvin_amd import ops
    args = _inputs(5000, 64, 3000, seed=11)
    item, s, _ = ops.l2_tail(*args)
    ri, rs, _ = _reference(*args)
    c = flash_results["legacy_D64_B5000_seed11"]
    for kernel, gi, gs in (("tile image", item, s), ("flash", torch.from_numpy(c["item_emb"]).to(DEV), torch.from_numpy(c["scores"]).to(DEV))):
        assert float((gi.double() - ri).abs().max()) < 1e-5 and float((gs.double() - rs).abs().max()) < 2e-5, kernel
    assert_close(c["item_emb"], item.cpu().numpy(), "flash tail vs tile-image kernel", rtol=1e-5, atol=2e-6)
    assert_close(c["scores"], s.cpu().numpy(), "scores, flash tail vs tile-image kernel", rtol=1e-5, atol=4e-6)


# ----------------------------------------------------------------------------------------------- the case list
def test_the_case_list_covers_what_it_claims(flash_results):
    assert set(flash_results) == set(tw.CASES)
    for fam, Bs in (("exact", {D: tw.B_LIST for D in tw.DIMS}), ("real", {16: tw.B_SUBSET, 32: tw.B_SUBSET, 64: tw.B_LIST})):
        for D in tw.DIMS:
            specs = [dict(tw.DEFAULTS, **tw.CASES[n]) for n in names_of(fam, D)]
            assert {s["B"] for s in specs} >= set(Bs[D])
            if D == 64:
                assert {s["B"] for s in specs if tw.flash_applies(s)} >= set(Bs[D]), "every batch size through the flash kernel"
            if fam == "exact":
                for opt in (dict(i64=False), dict(bias=False), dict(proj=False), dict(uo_is_q=True), dict(bf16=True), dict(null="both"),
                            dict(null="item"), dict(null="sig")):
                    assert any(all(s[k] == v for k, v in opt.items()) for s in specs), (D, opt)


@pytest.mark.parametrize("D", tw.DIMS)
def test_exact_cases_equal_float64_bit_for_bit(D, hip_lib, flash_results):
    fails, n = [], 0
    for name in names_of("exact", D):
        p, c = parent_result(name), flash_results[name]
        check(name, p, False, fails)
        check(name, c, True, fails)
        if not same(p, c):
            fails.append(f"{name}: the child's bits differ from the parent's")
        n += 1
    print(f"MEASURED exact cases at dim {D}: {n}, each in both processes")
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("D", tw.DIMS)
def test_real_cases_against_float64(D, hip_lib, flash_results):
    fails = []
    for name in names_of("real", D):
        if name.endswith("_walk"):
            continue
        check(name, parent_result(name), False, fails)
        check(name, flash_results[name], True, fails)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", [n for n in tw.CASES if n.endswith("_walk")])
def test_a_workgroup_walks_more_than_one_tile(name, hip_lib, flash_results):
    """More tiles than the persistent grid takes in one sweep: the loads issued a tile ahead are used."""
    s = tw.CASES[name]
    if s["D"] == 64:
        assert -(-tw.FLASH_WALK_B // 16) > 256 * 12 and -(-tw.TILE_WALK_B // 32) > 256 * 4
    else:
        assert -(-tw.TILE_WALK_B_SMALL // 32) > 256 * 8
    fails = []
    check(name, parent_result(name), False, fails)
    check(name, flash_results[name], True, fails)
    report()
    assert not fails, "\n".join(fails)


def test_the_child_ran_the_flash_kernel(hip_lib, flash_results):
    """Exact cases are bit-equal between the kernels by construction; the real-valued ones are not: the flash kernel starts its
    accumulators from the bias and sums a score over another tree."""
    names = [n for n in names_of("real", 64) if tw.flash_applies(tw.CASES[n])]
    assert len(names) >= len(tw.B_LIST)
    differ = sum(not same(parent_result(n), flash_results[n]) for n in names)
    print(f"MEASURED flash: dim-64 / fp32 / W0 real-valued cases that differ in some bit from the tile-image result: {differ} of {len(names)}")
    assert differ > 0, "every real-valued result of the child has the bits of the tile-image kernel: MVIN_TAIL_FLASH=1 was not honoured"


def test_the_child_keeps_the_tile_image_kernel_where_flash_declines(hip_lib, flash_results):
    """l2_tail_flash_applies declines dim 16 / 32, a bf16 table and W0 = None: both processes run the same kernel, bit for bit."""
    names = [n for n in tw.CASES if not n.startswith("legacy") and not tw.flash_applies(tw.CASES[n])]
    kinds = {(tw.CASES[n]["D"], bool(tw.CASES[n].get("bf16")), tw.CASES[n].get("proj", True)) for n in names}
    assert {(16, False, True), (32, False, True), (64, True, True), (64, False, False)} <= kinds
    bad = [n for n in names if not same(parent_result(n), flash_results[n])]
    print(f"MEASURED declined cases, bit-equal between the processes: {len(names) - len(bad)} of {len(names)}")
    assert not bad, f"the child's bits differ where the flash kernel does not apply: {bad}"


@pytest.mark.parametrize("name", names_of("ids"))
def test_ids_are_read_whole_and_clamped(name, hip_lib, flash_results):
    """Negative ids and ids with a high word read the table's LAST row: the bits of the same call with the ids clamped on the host."""
    fails = []
    for child, res in ((False, parent_result(name)), (True, flash_results[name])):
        if not same(res, res["clamped"]):
            case = references(name)[0]
            rows = np.nonzero((res["scores"].view(np.int32) != res["clamped"]["scores"].view(np.int32)))[0]
            fails.append(f"{name} [{kernel_of(name, child)}]: ids {sorted(set(int(case.items[r]) for r in rows))} are not read as the last row")
        check(name, res["clamped"], child, fails)
    assert not fails, "\n".join(fails)
