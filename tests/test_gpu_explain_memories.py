"""-m gpu: mvin_explain_memories on synthetic tables (200 entities, 7 relations, 40 users, at most 257 pairs).

ARITHMETIC.  out_probs, out_slot_contrib, out_block and out_bias against float64 (explain_memories_oracle.arith_oracle).  The
yardstick is the same formulas written the plain numpy way in float32; its error against float64 is measured on this module's own
inputs as one maximum per quantity (a maximum over many elements is a stable statistic; the error of one small case is not).  The
kernel may have at most 4 x that error -- the factor covers another summation order and another exp -- with a floor of 2^-23 in
the quantity's unit:
  probs         |err|                                   (a probability is at most 1)
  slot_contrib  |err| / max(1, largest |x_m . g_c| of the task)       (c_m = p_m * a_m with p_m <= 1)
  block         the same unit                           (the probabilities of a block sum to 1)
  bias          |err| / max(1, sum_i |bias_i * v_i|)
SELECTION.  Everything that is merging and ranking against oracle (a) applied to the kernel's OWN out_probs / out_slot_contrib:
bit for bit, the float32 sums included (their order is part of the rule).
Outputs sit between guard bytes; every launch checks them."""
import numpy as np
import pytest
import torch

from mvin_amd import ops
from explain_memories_oracle import arith_oracle, rank_oracle
from explain_oracle import explain_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
N_ENTITY, N_REL, N_USER = 200, 7, 40
FLOOR = 2.0 ** -23
KINDS = ("equal", "distinct", "half", "dyadic", "h_same", "edges", "garbage")
RANKED = ("mem", "mass", "contrib", "slot", "distinct", "total", "block")
QUANTITIES = ("probs", "slot_contrib", "block", "bias")

# (Nm, D, P, h-set block): every Nm at D = 8, every D at Nm = 16, every (P, w_h) that has a block
SHAPES = sorted({(Nm, 8, 1, True) for Nm in (1, 2, 5, 16, 33, 64)} | {(16, D, 1, True) for D in (4, 8, 16, 64, 128)}
                | {(16, 8, P, ft) for P in (0, 1, 2) for ft in (True, False) if P or ft})


def pairs_for(kind):
    return 257 if kind == "half" else 37                     # more than one workgroup tile, odd; one kind at the largest batch


def make(kind, shape, B, seed):
    """A case: tables, ripple sets of ``kind`` and per-pair inputs, all float32 / int32 numpy."""
    Nm, D, P, ft = shape
    rng = np.random.default_rng([seed, Nm, D, P, int(ft), KINDS.index(kind)])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    if kind == "dyadic":                                       # logits are exact small dyadic numbers: equal logits, equal probabilities
        E = rng.integers(-2, 3, (N_ENTITY, D)) / 4.0
        V = rng.integers(-2, 3, (B, N_REL, D)) / 4.0
        w_h = rng.integers(-2, 3, D) / 4.0
    else:
        E, V, w_h = rng.normal(0, 0.5, (N_ENTITY, D)), rng.normal(0, 0.5, (B, N_REL, D)), rng.normal(0, 0.5, D)
    Pm = max(1, P)
    h, t = rng.integers(0, N_ENTITY, (N_USER, Pm, Nm)), rng.integers(0, N_ENTITY, (N_USER, Pm, Nm))
    r = rng.integers(0, N_REL, (N_USER, Pm, Nm))
    users = rng.integers(0, N_USER, B)
    if kind == "equal":                                        # one memory in every slot
        h, r, t = (np.repeat(a[:, :, :1], Nm, axis=2) for a in (h, r, t))
    elif kind == "distinct":                                   # no two slots share an h
        h = np.stack([np.stack([rng.permutation(N_ENTITY)[:Nm] for _ in range(Pm)]) for _ in range(N_USER)])
    elif kind == "half":                                       # the upper half repeats the lower
        for a in (h, r, t):
            a[:, :, Nm - Nm // 2:] = a[:, :, :Nm // 2]
    elif kind == "dyadic":                                     # few entities and relations: duplicates AND ties between different keys
        h, t, r = h % 6, t % 6, r % 2
    elif kind == "h_same":                                     # h equal, t different: one memory in the h-set block, many in a hop block
        h, r = np.repeat(h[:, :, :1], Nm, axis=2), np.repeat(r[:, :, :1], Nm, axis=2)
        t = np.stack([np.stack([rng.permutation(N_ENTITY)[:Nm] for _ in range(Pm)]) for _ in range(N_USER)])
    elif kind == "edges":                                      # the first and the last row of the table
        h, t = np.where(h % 2 == 0, 0, N_ENTITY - 1), np.where(t % 3 == 0, 0, N_ENTITY - 1)
        r = np.where(r % 2 == 0, 0, N_REL - 1)
    elif kind == "garbage":                                    # ids out of range and negative: clamped for reads, reported raw
        bad = lambda a, lim: np.where(rng.random(a.shape) < 0.3, rng.choice([-1, -7, lim, lim + 5, 2 ** 31 - 1, -2 ** 31], a.shape), a)
        h, t, r = bad(h, N_ENTITY), bad(t, N_ENTITY), bad(r, N_REL)
        users = np.where(rng.random(B) < 0.3, rng.choice([-1, -2 ** 40, N_USER, N_USER + 3, 2 ** 40], B), users)
    uts = np.ascontiguousarray(np.stack([h, r, t], axis=2), dtype=np.int32)
    n_o = P + int(ft)
    return dict(kind=kind, shape=shape, E=f32(E), V=f32(V) if P else None, w_h=f32(w_h) if ft else None, uts=uts,
                users=np.ascontiguousarray(users, dtype=np.int64), G=f32(rng.normal(0, 0.5, (B, n_o * D))),
                bias=f32(rng.normal(0, 0.5, D)), item=f32(rng.normal(0, 0.5, (B, D))))


_cases = {}


def case_of(kind, shape, seed=1):
    """The case and its float64 reference, made once and shared (never modified)."""
    key = (kind, shape, seed)
    if key not in _cases:
        c = make(kind, shape, pairs_for(kind), seed)
        c["ref"] = arith(c, np.float64)
        _cases[key] = c
    return _cases[key]


def arith(c, dtype):
    return arith_oracle(c["E"], c["V"], c["w_h"], c["uts"], c["users"], c["G"], c["bias"], c["item"], c["shape"][2], dtype)


def errors(got, c):
    """The largest error of each quantity against the case's float64 reference, in the quantity's unit."""
    ref = c["ref"]
    unit = np.maximum(1.0, np.abs(ref["value"]).max(axis=-1))                              # [B, n_o]
    bias_unit = np.maximum(1.0, (np.abs(c["bias"].astype(np.float64))[None, :] * np.abs(c["item"].astype(np.float64))).sum(axis=-1))
    return dict(probs=np.abs(got["probs"] - ref["probs"]).max(),
                slot_contrib=(np.abs(got["slot_contrib"] - ref["slot_contrib"]) / unit[:, :, None]).max(),
                block=(np.abs(got["block"] - ref["block"]) / unit).max(), bias=(np.abs(got["bias"] - ref["bias"]) / bias_unit).max())


@pytest.fixture(scope="module")
def yardstick():
    """quantity -> the float32 yardstick's largest error over every (shape, kind) of this module; computed once."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for shape in SHAPES:
        for kind in KINDS:
            c = case_of(kind, shape)
            e = errors(arith(c, np.float32), c)
            worst = {q: max(worst[q], float(e[q])) for q in QUANTITIES}
    print("float32 yardstick: " + "  ".join(f"{q} {worst[q]:.3e}" for q in QUANTITIES))
    return worst


class Guarded(object):
    """An output tensor inside a larger buffer of sentinel values."""
    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.sentinel = -0x5A5A5A5A5A if dtype == torch.int64 else -0x5A5A5A              # exact in float32 too
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[-GUARD:] == self.sentinel).all())


def run(c, top, profile=True, rel_mass=None, sel=None, want_slots=True):
    """One launch on guarded outputs -> dict of numpy arrays (and the guarded rel_mass)."""
    Nm, D, P, ft = c["shape"]
    users, G, item, V = c["users"], c["G"], c["item"], c["V"]
    if sel is not None:
        users, G, item, V = users[sel], G[sel], item[sel], None if V is None else V[sel]
    B, n_o = users.shape[0], P + int(ft)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    outs = dict(mem=Guarded((B, n_o, top, 3), i32), mass=Guarded((B, n_o, top), i64), contrib=Guarded((B, n_o, top), f32),
                slot=Guarded((B, n_o, top), i32), distinct=Guarded((B, n_o), i32), total=Guarded((B, n_o), i64),
                block=Guarded((B, n_o), f32), bias=Guarded((B,), f32))
    if want_slots:
        outs.update(probs=Guarded((B, n_o, Nm), f32), slot_contrib=Guarded((B, n_o, Nm), f32))
    profile = profile and P > 0
    if profile and rel_mass is None:
        rel_mass = Guarded((P, N_REL), i64, fill=0)
    ops.explain_memories(dev(c["E"]), dev(V), dev(c["w_h"]), dev(c["uts"]), dev(users), dev(G), dev(c["bias"]), dev(item), P, top,
                         rel_mass=rel_mass.t if profile else None, want_slots=want_slots, out={k: g.t for k, g in outs.items()})
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs.values()), "an output's guard values were overwritten"
    assert not profile or rel_mass.intact(), "rel_mass' guard values were overwritten"
    res = {k: g.t.cpu().numpy() for k, g in outs.items()}
    res["rel_mass"] = rel_mass.t.cpu().numpy() if profile else None
    res["rel_mass_buf"] = rel_mass
    return res


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, top=None, what="", names=RANKED):
    for n in names:
        w = want[n] if top is None or want[n].ndim < 3 else want[n][:, :, :top]
        assert got[n].dtype == w.dtype and np.array_equal(bits(got[n]), bits(w)), (what, n)


def oracle_on(got, c, top, sel=None):
    users = c["users"] if sel is None else c["users"][sel]
    return rank_oracle(got["probs"], got["slot_contrib"], c["uts"], users, c["shape"][2], c["shape"][3], top, n_relation=N_REL)


def check_kind(got, want, c):
    """What a kind of ripple set must show, so that a case that lost its point fails."""
    kind, (Nm, D, P, ft) = c["kind"], c["shape"]
    hop = slice(1 if ft else 0, None)
    if kind == "equal":                                        # one memory whose mass is the total
        assert (want["distinct"] == 1).all() and np.array_equal(got["mass"][:, :, 0], got["total"]) and (got["slot"][:, :, 0] == 0).all()
        assert (got["slot"][:, :, 1:] == -1).all() and (got["mass"][:, :, 1:] == 0).all() and (got["mem"][:, :, 1:] == -1).all()
        assert np.array_equal(bits(got["contrib"][:, :, 0]), bits(got["block"]))
    if kind == "distinct":
        assert (want["distinct"] == Nm).all()
    if kind == "half" and Nm >= 2:
        assert want["distinct"].max() <= Nm - Nm // 2
    if kind == "dyadic" and Nm >= 16 and P:                    # a hop logit is one number per (h, r): memories that differ in t alone
        m = got["mass"][:, hop]                                # tie exactly -- equal masses side by side
        assert ((m[:, :, :-1] == m[:, :, 1:]) & (m[:, :, 1:] > 0)).any()
    if kind == "h_same":
        if ft:
            assert (want["distinct"][:, 0] == 1).all()
        if P:
            assert (want["distinct"][:, hop] == Nm).all()
    if kind == "edges":
        assert set(np.unique(got["mem"][:, :, :, 0])) <= {0, N_ENTITY - 1, -1} and want["distinct"].max() <= 8
    if kind == "garbage":                                      # raw ids come back
        assert got["mem"].min() < -1 and got["mem"].max() >= N_ENTITY
    if ft:
        assert (got["mem"][:, 0, :, 1:] == -1).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"Nm{s[0]}-D{s[1]}-P{s[2]}-{'hset' if s[3] else 'nohset'}")
def test_kernel_against_float64_and_selection_oracle(hip_lib, yardstick, shape):
    Nm, D, P, ft = shape
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for kind in KINDS:
        c = case_of(kind, shape)
        got = run(c, Nm)
        e = errors(got, c)
        worst = {q: max(worst[q], float(e[q])) for q in QUANTITIES}
        for q in QUANTITIES:
            assert e[q] <= max(4.0 * yardstick[q], FLOOR), f"{kind}: {q} error {e[q]:.3e}, float32 yardstick {yardstick[q]:.3e}"
        want = oracle_on(got, c, Nm)
        same(got, want, what=kind)
        if P:
            assert np.array_equal(got["rel_mass"], want["rel_mass"]), kind
        # every memory is listed: the masses add up to the total, the listed rows are the distinct ones
        assert np.array_equal(got["mass"].sum(axis=2), got["total"]) and np.array_equal((got["slot"] >= 0).sum(axis=2), got["distinct"])
        check_kind(got, want, c)
        for top in sorted({1, min(5, Nm)} - {Nm}):             # a smaller top is a prefix; the optional outputs may be left out
            less = run(c, top, profile=False, want_slots=False)
            same(less, want, top, (kind, top))
            assert np.array_equal(bits(less["bias"]), bits(got["bias"]))
    print(f"Nm={Nm} D={D} P={P} hset={ft}: kernel " + "  ".join(f"{q} {worst[q]:.3e}" for q in QUANTITIES)
          + "  (yardstick " + "  ".join(f"{yardstick[q]:.3e}" for q in QUANTITIES) + ")")


def test_every_top_at_five_memories(hip_lib):
    shape = (5, 8, 1, True)
    for kind in KINDS:
        c = case_of(kind, shape)
        full = run(c, 5)
        want = oracle_on(full, c, 5)
        same(full, want, what=kind)
        for top in range(1, 5):
            got = run(c, top)
            same(got, want, top, (kind, top))
            assert np.array_equal(got["rel_mass"], want["rel_mass"]) and np.array_equal(bits(got["probs"]), bits(full["probs"]))


@pytest.mark.parametrize("shape", [(16, 8, 2, True), (33, 16, 1, False), (64, 64, 2, True)], ids=str)
def test_pair_alone_elsewhere_and_launch_shape(hip_lib, monkeypatch, shape):
    """A row is a pure function of its pair: alone (B = 1), at another position, again, and under a grid of 1 or 3 workgroups."""
    names = RANKED + ("bias", "probs", "slot_contrib")
    for kind in ("half", "garbage"):
        c = case_of(kind, shape, seed=2)
        B, top = c["users"].shape[0], min(7, shape[0])
        full = run(c, top)
        again = run(c, top)
        same(again, full, what="second run", names=names)
        assert np.array_equal(again["rel_mass"], full["rel_mass"])
        for b in (0, B // 2, B - 1):
            alone = run(c, top, sel=slice(b, b + 1))
            for n in names:
                assert np.array_equal(bits(alone[n][0]), bits(full[n][b])), (kind, b, n)
        order = np.arange(B)[::-1].copy()                      # every pair at another position, in other company per workgroup
        moved = run(c, top, sel=order)
        for n in names:
            assert np.array_equal(bits(moved[n]), bits(full[n][order])), (kind, "moved", n)
        assert np.array_equal(moved["rel_mass"], full["rel_mass"])
        for wgs in ("1", "3"):
            monkeypatch.setenv("MVIN_EXPLAIN_MEM_WGS", wgs)
            capped = run(c, top)
            monkeypatch.delenv("MVIN_EXPLAIN_MEM_WGS")
            same(capped, full, what=("grid", wgs), names=names)
            assert np.array_equal(capped["rel_mass"], full["rel_mass"]), wgs
        same(run(c, top, profile=False), full, what="without rel_mass", names=names)


def test_profile_accumulates(hip_lib):
    c = case_of("half", (16, 8, 2, True))
    once = run(c, 1)
    want = oracle_on(once, c, 1)
    twice = run(c, 1, rel_mass=once["rel_mass_buf"])           # accumulated into the same buffer
    assert np.array_equal(once["rel_mass"], want["rel_mass"]) and np.array_equal(twice["rel_mass"], 2 * want["rel_mass"])
    # every relation id is in range: a hop's row is the sum of its blocks' totals
    assert np.array_equal(want["rel_mass"].sum(axis=1), want["total"][:, 1:].sum(axis=0))
    g = case_of("garbage", (16, 8, 2, True))
    got = run(g, 1)
    want = oracle_on(got, g, 1)
    assert np.array_equal(got["rel_mass"], want["rel_mass"]) and (want["rel_mass"].sum(axis=1) < want["total"][:, 1:].sum(axis=0)).all()


def test_explain_paths_is_untouched_by_the_shared_header(hip_lib):
    """mvin_explain_paths on a fixed input gives the same bytes before and after a launch of the new kernel in this process,
    and they are the oracle's."""
    rng = np.random.default_rng(8)
    B, K, nR = 33, 8, 5
    imp0, imp1 = rng.random((B, 1, K)).astype(np.float32), rng.random((B, K, K)).astype(np.float32)
    rel0, ent1 = rng.integers(0, nR, (B, K)).astype(np.int32), rng.integers(0, 6, (B, K)).astype(np.int32)
    rel1, ent2 = rng.integers(0, nR, (B, K * K)).astype(np.int32), rng.integers(0, 6, (B, K * K)).astype(np.int32)
    dev = lambda a: torch.from_numpy(a).to(DEV)

    def paths():
        rel_mass = torch.zeros((2, nR), dtype=torch.int64, device=DEV)
        out = ops.explain_paths(dev(imp0), dev(imp1), [dev(rel0), dev(rel1)], [None, dev(ent1), dev(ent2)], 6, nR, rel_mass=rel_mass)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out + (rel_mass,)]
    before = paths()
    run(case_of("half", (16, 8, 2, True)), 3)
    after = paths()
    want = explain_oracle(imp0, imp1, rel0, ent1, rel1, ent2, 6, n_relation=nR)
    for a, b, n in zip(before, after, ("paths", "mass", "slot", "distinct", "total", "rel_mass")):
        assert a.tobytes() == b.tobytes() and np.array_equal(a, want[n]), n


def test_empty_batch_and_refusals(hip_lib):
    c = case_of("half", (16, 8, 2, True))
    got = run(c, 3, sel=slice(0, 0))
    assert got["mem"].shape == (0, 3, 3, 3) and (got["rel_mass"] == 0).all()
    dev = lambda a: torch.from_numpy(a).to(DEV)
    a = [dev(c[k]) for k in ("E", "V", "w_h", "uts", "users", "G", "bias", "item")]
    with pytest.raises(ValueError, match="top=17"):
        ops.explain_memories(*a, 2, 17)
    with pytest.raises(ValueError, match="rel_mass"):
        ops.explain_memories(*a, 2, 3, rel_mass=torch.zeros((2, 5), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="fp32"):
        ops.explain_memories(a[0].to(torch.bfloat16), *a[1:], 2, 3)
    with pytest.raises(ValueError, match="out"):
        ops.explain_memories(*a, 2, 3, out=dict(mem=torch.empty((1, 3, 3, 3), dtype=torch.int32, device=DEV)))
