"""-m gpu: mvin_explain_paths bit for bit against the numpy oracle (tests/explain_oracle.py) on synthetic inputs, for every
fan-out at which the kernel takes another path -- K*K <= 64: a pair per lane group of 2 .. 64 lanes; beyond: a workgroup per pair
over 256, 1 024 or 4 096 padded entries -- in both modes, with guard bytes around every output."""
import numpy as np
import pytest
import torch

from mvin_amd import ops
from explain_oracle import explain_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 2, 4, 8, 16, 32, 64)
KINDS = ("merge", "few", "distinct", "equal", "garbage", "large", "oor")
GUARD = 64
OUT_NAMES = ("paths", "mass", "slot", "distinct", "total")


def pairs_for(K, two):
    """B <= 300, and about 50 000 entries at most so that the oracle stays quick; more than one workgroup everywhere."""
    return 300 if (K <= 8 or not two) else {16: 150, 32: 40, 64: 12}[K]


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def make(kind, B, K, two, seed):
    """(imp0 [B,1,K], imp1 [B,K,K] or None, rel0, ent1, rel1, ent2, n_relation) as numpy arrays."""
    rng = np.random.default_rng([seed, K, int(two), KINDS.index(kind)])
    N = K * K
    n_relation = 4
    imp0 = softmax(rng.normal(size=(B, 1, K)))
    imp1 = softmax(rng.normal(size=(B, K, K)))
    rel0, rel1 = rng.integers(0, 2, (B, K)), rng.integers(0, 2, (B, N))
    ent1, ent2 = rng.integers(100, 103, (B, K)), rng.integers(100, 103, (B, N))                # 3 entities, 2 relations
    if kind == "few":                                         # every slot identical: one path that carries everything
        rel0[:], rel1[:], ent1[:], ent2[:] = 1, 2, 7, 9
        imp0[:], imp1[:] = np.float32(1 / K), np.float32(1 / K)
    elif kind in ("distinct", "equal"):                       # no merging at all
        ent1 = np.tile(np.arange(K), (B, 1)) + 1000
        ent2 = rng.permuted(np.tile(np.arange(N), (B, 1)), axis=1)
        if kind == "equal":                                   # ... and equal weights: pure slot order
            imp0[:], imp1[:] = np.float32(1 / K), np.float32(1 / K)
    elif kind == "garbage":
        junk = np.float32([np.nan, np.inf, -np.inf, -1.0, 2.0, 1e-40, 0.0, -0.0, 1.0, 3e-39])
        for w in (imp0, imp1):
            hit = rng.random(w.shape) < 0.3
            w[hit] = junk[rng.integers(0, len(junk), int(hit.sum()))]
        w = imp0.view(np.uint32)                              # ... and NaNs with payloads and sign bits
        w[rng.random(w.shape) < 0.05] = np.uint32(0xFFC12345)
    elif kind == "large":                                     # ids at the ends of their ranges; more relations than LDS bins
        n_relation = 1000
        rel0, rel1 = rng.choice([0, 999, 998], (B, K)), rng.choice([0, 999, 500], (B, N))
        ent1 = rng.choice([2 ** 31 - 1, 2 ** 31 - 2, 0], (B, K))
        ent2 = rng.choice([2 ** 31 - 1, 2 ** 31 - 2, 0, 1], (B, N))
    elif kind == "oor":                                       # relation ids outside [0, n_relation), ids that do not fit the key
        rel0, rel1 = rng.integers(-3, n_relation + 3, (B, K)), rng.integers(-3, n_relation + 3, (B, N))
        far = rng.random((B, N)) < 0.1
        rel1[far] = rng.choice([2 ** 25, 2 ** 25 - 1, 2 ** 31 - 1, -2 ** 31], int(far.sum()))
        ent2[rng.random((B, N)) < 0.1] = -1
        ent1[rng.random((B, K)) < 0.2] = -7
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    if not two:
        return imp0, None, i32(rel0), i32(ent1), None, None, n_relation
    return imp0, imp1, i32(rel0), i32(ent1), i32(rel1), i32(ent2), n_relation


class Guarded(object):
    """An output tensor inside a larger buffer of sentinel bytes."""
    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.sentinel = -0x5A5A5A5A5A if dtype == torch.int64 else -0x5A5A5A
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[-GUARD:] == self.sentinel).all())


def run(case, top, profile=True, rel_mass=None, sel=None):
    """One launch on guarded outputs -> dict of numpy arrays (and the guarded rel_mass)."""
    imp0, imp1, rel0, ent1, rel1, ent2, nR = case
    if sel is not None:
        imp0, rel0, ent1 = imp0[sel], rel0[sel], ent1[sel]
        imp1, rel1, ent2 = (imp1[sel], rel1[sel], ent2[sel]) if imp1 is not None else (None, None, None)
    B = imp0.shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    outs = [Guarded((B, top, 4), torch.int32), Guarded((B, top), torch.int64), Guarded((B, top), torch.int32),
            Guarded((B,), torch.int32), Guarded((B,), torch.int64)]
    if profile and rel_mass is None:
        rel_mass = Guarded((2, nR), torch.int64, fill=0)
    ops.explain_paths(dev(imp0), dev(imp1), [dev(rel0), dev(rel1)], [None, dev(ent1), dev(ent2)], top, nR,
                      rel_mass=rel_mass.t if rel_mass is not None else None, out=tuple(g.t for g in outs))
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs), "an output's guard bytes were overwritten"
    assert rel_mass is None or rel_mass.intact(), "rel_mass' guard bytes were overwritten"
    res = {n: g.t.cpu().numpy() for n, g in zip(OUT_NAMES, outs)}
    res["rel_mass"] = rel_mass.t.cpu().numpy() if rel_mass is not None else None
    res["rel_mass_buf"] = rel_mass
    return res


def same(got, want, top=None, what=""):
    for n in OUT_NAMES:
        w = want[n] if top is None or n in ("distinct", "total") else want[n][:, :top]
        assert got[n].dtype == w.dtype and np.array_equal(got[n], w), (what, n)


@pytest.mark.parametrize("two", (True, False), ids=("two_hop", "one_hop"))
@pytest.mark.parametrize("K", KS)
def test_kernel_equals_oracle(hip_lib, K, two):
    """Every kind of input x top in {1, 5, all entries}: paths, masses, slots, distinct counts, totals and the profile."""
    B, N = pairs_for(K, two), K * K if two else K
    for kind in KINDS:
        case = make(kind, B, K, two, seed=1)
        want = explain_oracle(*case[:6], top=N, n_relation=case[6])            # a smaller top is a prefix of its rows
        assert want["distinct"].max() <= N and (kind != "few" or (want["distinct"] == 1).all())
        assert kind not in ("distinct", "equal") or (want["distinct"] == N).all()
        for top in sorted({1, min(5, N), N}):
            got = run(case, top)
            same(got, want, top, (kind, top))
            assert np.array_equal(got["rel_mass"], want["rel_mass"]), (kind, top)
            if top == N:                                      # every path is listed: the masses add up to the total
                assert np.array_equal(got["mass"].sum(axis=1), got["total"]), kind
                assert ((got["slot"] >= 0).sum(axis=1) == got["distinct"]).all(), kind
        if kind == "few":
            got = run(case, min(3, N))
            assert (got["mass"][:, 0] == got["total"]).all() and (got["slot"][:, 0] == 0).all() and (got["slot"][:, 1:] == -1).all()
        most = 36 if two else 6                               # 2 relations x 3 entities per level
        if kind == "merge" and N > most:                      # top = N beyond the distinct count: padding rows
            assert want["distinct"].max() <= most and (got["paths"][:, most:] == -1).all() and (got["mass"][:, most:] == 0).all()


@pytest.mark.parametrize("two", (True, False), ids=("two_hop", "one_hop"))
@pytest.mark.parametrize("K", (2, 8, 16, 64))
def test_pair_alone_repeat_and_launch_shape(hip_lib, monkeypatch, K, two):
    """A row is a pure function of its pair: alone (B = 1), inside the batch, again, and under a grid of 1 or 3 workgroups."""
    B, N = pairs_for(K, two), K * K if two else K
    top = min(7, N)
    for kind in ("merge", "garbage"):
        case = make(kind, B, K, two, seed=2)
        full = run(case, top)
        same(run(case, top), full, what="second run")
        assert np.array_equal(run(case, top)["rel_mass"], full["rel_mass"])
        for b in (0, B // 2, B - 1):
            alone = run(case, top, sel=slice(b, b + 1))
            for n in OUT_NAMES:
                assert np.array_equal(alone[n][0], full[n][b]), (kind, b, n)
        for wgs in ("1", "3"):
            monkeypatch.setenv("MVIN_EXPLAIN_WGS", wgs)
            capped = run(case, top)
            monkeypatch.delenv("MVIN_EXPLAIN_WGS")
            same(capped, full, what=("grid", wgs))
            assert np.array_equal(capped["rel_mass"], full["rel_mass"]), wgs
        no_profile = run(case, top, profile=False)
        same(no_profile, full, what="without rel_mass")


@pytest.mark.parametrize("K", (4, 32))
def test_profile_accumulates_and_sums_to_total(hip_lib, K):
    B = pairs_for(K, True)
    case = make("merge", B, K, True, seed=3)
    want = explain_oracle(*case[:6], top=1, n_relation=case[6])
    once = run(case, 1)
    twice = run(case, 1, rel_mass=once["rel_mass_buf"])       # accumulated into the same buffer
    assert np.array_equal(once["rel_mass"], want["rel_mass"]) and np.array_equal(twice["rel_mass"], 2 * want["rel_mass"])
    # level 1 adds floor(w0 * 2^40) per slot, level 2 the path-slot masses: with every id in range row 1 is the batch's total
    assert want["rel_mass"][1].sum() == want["total"].sum()
    for b in (0, B - 1):
        alone = run(case, 1, sel=slice(b, b + 1))
        assert alone["rel_mass"][1].sum() == alone["total"][0] == want["total"][b]
    for kind in ("large", "oor"):                             # relations beyond the LDS bins; ids out of range add nothing
        case = make(kind, B, K, True, seed=3)
        got, want = run(case, 1), explain_oracle(*case[:6], top=1, n_relation=case[6])
        assert np.array_equal(got["rel_mass"], want["rel_mass"]), kind
    assert want["rel_mass"][1].sum() < want["total"].sum()    # "oor": the out-of-range relations are in the total, not the profile


def test_empty_batch_and_refusals(hip_lib):
    case = make("merge", 0, 4, True, seed=4)
    got = run(case, 3)
    assert got["paths"].shape == (0, 3, 4) and (got["rel_mass"] == 0).all()
    case = make("merge", 2, 4, True, seed=4)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    args = (dev(case[0]), dev(case[1]), [dev(case[2]), dev(case[4])], [None, dev(case[3]), dev(case[5])])
    with pytest.raises(ValueError, match="top"):
        ops.explain_paths(*args, 17, 4)
    with pytest.raises(ValueError, match="rel_mass"):
        ops.explain_paths(*args, 3, 4, rel_mass=torch.zeros((2, 5), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="expected"):
        ops.explain_paths(args[0], args[1], [args[2][0], args[2][1][:, :8].contiguous()], args[3], 3, 4)
