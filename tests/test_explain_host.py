"""CPU: explaining a score (mvin_explain_paths, ops.explain_paths, DeviceFeeder.explain, harness.explain_pairs /
relation_profile) where no GPU is needed -- the oracle the GPU tests compare against, checked by hand; the mass definition
against exact rational arithmetic, and the bit-field form the kernel computes it in; the ABI's symbols and refusals before any
launch; the refusal of CPU tensors; the records and shares of the harness on a stubbed feeder."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from mvin_amd import harness, ops
from explain_oracle import clean, explain_oracle, mass1, mass2, slot_masses

ONE = 1 << 40


# --------------------------------------------------------------------------- the oracle, by hand
def test_oracle_by_hand_two_hops():
    """K = 2, three pairs.  Pair 0: a duplicated level-1 slot whose paths merge into two paths of EQUAL mass (slot decides) and
    fewer distinct paths than ``top``.  Pair 1: a NaN, a negative and a 2.0 weight.  Pair 2: slots that do not fit the key."""
    nan = np.nan
    imp0 = np.float32([[0.5, 0.25], [nan, 2.0], [0.5, 0.5]]).reshape(3, 1, 2)
    imp1 = np.float32([[[0.5, 0.5], [0.5, 0.5]], [[0.5, 0.5], [-1.0, 0.75]], [[0.5, 0.25], [0.125, 1.0]]])
    rel0 = np.int32([[1, 1], [0, 1], [-5, 2]])
    ent1 = np.int32([[7, 7], [4, 5], [6, 6]])
    rel1 = np.int32([[2, 3, 2, 3], [0, 1, 2, 3], [1 << 25, 0, 1, 1]])
    ent2 = np.int32([[9, 8, 9, 8], [10, 11, 12, 13], [3, 3, -1, 3]])
    o = explain_oracle(imp0, imp1, rel0, ent1, rel1, ent2, top=3, n_relation=3)
    q = ONE // 8
    # pair 0: slots 0 + 2 and 1 + 3 merge (level-1 slots 0 and 1 are the same edge): 3/8 each, the lower slot first, then padding
    assert o["paths"][0].tolist() == [[1, 7, 2, 9], [1, 7, 3, 8], [-1, -1, -1, -1]]
    assert o["mass"][0].tolist() == [3 * q, 3 * q, 0] and o["slot"][0].tolist() == [0, 1, -1]
    assert o["distinct"][0] == 2 and o["total"][0] == 6 * q
    # pair 1: NaN -> 0 kills slots 0 and 1, -1 -> 0 kills slot 2, 2.0 -> 1 leaves slot 3 with 0.75; zero paths follow by slot
    assert o["paths"][1].tolist() == [[1, 5, 3, 13], [0, 4, 0, 10], [0, 4, 1, 11]]
    assert o["mass"][1].tolist() == [6 * q, 0, 0] and o["slot"][1].tolist() == [3, 0, 1]
    assert o["distinct"][1] == 4 and o["total"][1] == 6 * q
    # pair 2: rel1 = 2^25 (slot 0) and ent2 = -1 (slot 2) do not fit: dropped.  A negative rel0 is compared as it is
    assert o["paths"][2].tolist() == [[2, 6, 1, 3], [-5, 6, 0, 3], [-1, -1, -1, -1]]
    assert o["mass"][2].tolist() == [4 * q, q, 0] and o["slot"][2].tolist() == [3, 1, -1]
    assert o["distinct"][2] == 2 and o["total"][2] == 5 * q
    # the profile: level 1 by rel0 (NaN adds 0, rel0 = -5 is out of range), level 2 by rel1 (3 and 2^25 are out of range)
    assert o["rel_mass"].tolist() == [[0, 6 * q + 8 * q, 4 * q], [q, 4 * q, 3 * q]]
    # the rows of a smaller ``top`` are a prefix
    o1 = explain_oracle(imp0, imp1, rel0, ent1, rel1, ent2, top=1)
    assert np.array_equal(o1["paths"], o["paths"][:, :1]) and np.array_equal(o1["mass"], o["mass"][:, :1]) and o1["rel_mass"] is None


def test_oracle_by_hand_one_hop():
    imp0 = np.float32([[0.25, 0.5, 0.25, np.inf]])
    rel0, ent1 = np.int32([[3, 1, 3, 0]]), np.int32([[8, 8, 8, 2]])
    o = explain_oracle(imp0, None, rel0, ent1, None, None, top=4, n_relation=4)
    h = ONE // 2
    # slots 0 and 2 merge to 0.5 = slot 1's mass: slot 0 goes first; +inf -> 0 is a path of mass 0
    assert o["paths"][0].tolist() == [[3, 8, -1, -1], [1, 8, -1, -1], [0, 2, -1, -1], [-1, -1, -1, -1]]
    assert o["mass"][0].tolist() == [h, h, 0, 0] and o["slot"][0].tolist() == [0, 1, 3, -1]
    assert o["distinct"][0] == 3 and o["total"][0] == ONE
    assert o["rel_mass"].tolist() == [[0, h, 0, h], [0, 0, 0, 0]]


# --------------------------------------------------------------------------- the mass definition
def _weights(rng, n):
    w = rng.random(n).astype(np.float32)
    w[::7] = rng.random(len(w[::7])).astype(np.float32) * np.float32(1e-38)          # denormals and near-denormals
    w[1::11] = np.float32(2.0 ** -rng.integers(1, 149, len(w[1::11])))
    w[2::13] = np.float32([1.0, np.nextafter(np.float32(1), np.float32(0)), 1.5, 0.0, -0.0, np.nan, np.inf, -np.inf, -0.3,
                           1e-45, 3e38])[rng.integers(0, 11, len(w[2::13]))]
    return w


def _mass_from_bits(b0, b1=None):
    """The kernel's form: a cleaned weight is M * 2^(E - 150) with a 24-bit M, the mass a product and a shift."""
    def field(bits):
        bits = int(bits)
        e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
        if bits >> 31 or e == 0xFF:
            return 0, 1
        if e >= 127:
            return 1 << 23, 127
        return (m, 1) if e == 0 else (m | 1 << 23, e)
    M0, E0 = field(b0)
    if b1 is None:
        sh = 110 - E0
        return M0 >> sh if sh >= 0 else M0 << -sh
    M1, E1 = field(b1)
    return (M0 * M1) >> (260 - E0 - E1)


def test_mass_is_exact_rational_arithmetic():
    rng = np.random.default_rng(5)
    w0, w1 = _weights(rng, 4000), _weights(rng, 4000)[::-1].copy()
    c0, c1 = clean(w0), clean(w1)
    assert np.isfinite(c0).all() and (c0 >= 0).all() and (c0 <= 1).all()
    assert c0[np.isnan(w0) | np.isinf(w0) | (w0 <= 0)].max() == 0 and (c0[w0 > 1][np.isfinite(w0[w0 > 1])] == 1).all()
    m2, m1 = mass2(w0, w1), mass1(w0)
    assert m2.dtype == np.int64 and m1.dtype == np.int64
    for i in range(len(w0)):
        f0, f1 = Fraction(float(c0[i])), Fraction(float(c1[i]))
        assert int(m2[i]) == (f0 * f1 * ONE).__floor__(), (w0[i], w1[i])
        assert int(m1[i]) == (f0 * ONE).__floor__(), w0[i]
        assert int(m2[i]) == _mass_from_bits(w0[i:i + 1].view(np.uint32)[0], w1[i:i + 1].view(np.uint32)[0]), (w0[i], w1[i])
        assert int(m1[i]) == _mass_from_bits(w0[i:i + 1].view(np.uint32)[0]), w0[i]
    assert mass1(np.float32([1.0, 7.0]))[0] == ONE == mass1(np.float32([1.0, 7.0]))[1] and mass2(np.float32(1), np.float32(1)) == ONE
    # a slot that does not fit the key has mass 0
    sm = slot_masses(np.float32([[1.0]]), np.float32([[[0.5]]]), np.int32([[1 << 25]]), np.int32([[0]]))
    assert sm.tolist() == [[0]]


# --------------------------------------------------------------------------- the C ABI
def _p(x):
    return None if x is None else C.c_void_p(x)


def _call(lib, imp0=16, imp1=16, rel0=16, ent1=16, rel1=16, ent2=16, B=4, K=8, top=5, n_relation=6, out_paths=16, out_mass=16,
          out_slot=16, out_distinct=16, out_total=16, rel_mass=None):
    return lib.mvin_explain_paths(_p(imp0), _p(imp1), _p(rel0), _p(ent1), _p(rel1), _p(ent2), B, K, top, n_relation, _p(out_paths),
                                  _p(out_mass), _p(out_slot), _p(out_distinct), _p(out_total), _p(rel_mass), None)


def test_explain_symbols_and_signatures(hip_lib):
    from mvin_amd import _lib
    for name in ("mvin_explain_paths", "mvin_explain_paths_max_k"):
        assert name in _lib.SIGNATURES
        assert getattr(hip_lib, name) is not None
    assert len(_lib.SIGNATURES["mvin_explain_paths"][1]) == 17
    assert hip_lib.mvin_explain_paths_max_k() == 64 == ops.explain_paths_max_k()
    assert hip_lib.mvin_abi_version() == 12


def test_explain_abi_validates_before_launching(hip_lib):
    # every failing call fails on the host: the fake device pointers are never dereferenced and nothing is launched
    one_hop = dict(imp1=None, rel1=None, ent2=None)
    null = [dict(imp0=None), dict(rel0=None), dict(ent1=None), dict(out_paths=None), dict(out_mass=None), dict(out_slot=None),
            dict(out_distinct=None), dict(out_total=None), dict(imp1=None), dict(rel1=None), dict(ent2=None),
            dict(imp1=None, rel1=None), dict(rel1=None, ent2=None), dict(imp1=None, ent2=None)]
    size = [dict(K=0), dict(K=65), dict(K=128), dict(K=-1), dict(top=0), dict(top=65), dict(top=-2), dict(top=9, **one_hop),
            dict(B=-1), dict(B=1 << 25), dict(B=(1 << 31) // 64), dict(n_relation=1 << 25), dict(n_relation=-1),
            dict(rel_mass=16, B=(1 << 22) // 64 + 1), dict(rel_mass=16, n_relation=0), dict(rel_mass=16, B=(1 << 16) + 1, **one_hop)]
    for code, cases in ((-1, null), (-2, size)):
        for kw in cases:
            assert _call(hip_lib, **kw) == code, kw
            assert b"mvin_explain_paths" in hip_lib.mvin_last_error(), kw
    # B == 0 is valid and launches nothing, in both modes, at the limits of every size
    assert _call(hip_lib, B=0) == 0 and _call(hip_lib, B=0, **one_hop) == 0
    assert _call(hip_lib, B=0, K=64, top=4096, n_relation=(1 << 25) - 1) == 0
    assert _call(hip_lib, B=0, K=64, top=64, **one_hop) == 0 and _call(hip_lib, B=0, K=1, top=1) == 0
    assert _call(hip_lib, B=0, rel_mass=16) == 0 and _call(hip_lib, B=0, n_relation=0) == 0


def test_explain_ops_refuse_cpu_tensors_and_bad_shapes(hip_lib):
    from mvin_amd import _lib
    K = 2
    imp0, imp1 = torch.full((3, 1, K), 0.5), torch.full((3, K, K), 0.5)
    ents = [torch.zeros((3, 1), dtype=torch.int32), torch.zeros((3, K), dtype=torch.int32), torch.zeros((3, K * K), dtype=torch.int32)]
    rels = [torch.zeros((3, K), dtype=torch.int32), torch.zeros((3, K * K), dtype=torch.int32)]
    with pytest.raises(_lib.MvinHipError):
        ops.explain_paths(imp0, imp1, rels, ents, 2, 5)
    with pytest.raises(_lib.MvinHipError):
        ops.explain_paths(imp0, None, rels, ents, 2, 5)


# --------------------------------------------------------------------------- the harness on a stubbed feeder
class _StubFeeder(object):
    """DeviceFeeder.explain replaced by the oracle on hand-made attention: what explain_pairs / relation_profile do with it."""
    def __init__(self, two=True):
        self.model = type("M", (), dict(n_mix_hop=1, h_hop=2 if two else 1))()
        self.two, self.calls = two, []

    def explain(self, users, items, top=10, profile=False, return_attention=False, max_pairs=65536):
        self.calls.append(dict(top=top, profile=profile, max_pairs=max_pairs))
        B, K = len(users), 2
        imp0 = np.tile(np.float32([[0.75, 0.25]]), (B, 1))
        imp1 = np.tile(np.float32([[[0.5, 0.5], [1.0, 0.0]]]), (B, 1, 1)) if self.two else None
        rel0, ent1 = np.tile(np.int32([[1, 2]]), (B, 1)), np.tile(np.int32([[10, 11]]), (B, 1))
        rel1, ent2 = (np.tile(np.int32([[0, 0, 2, 2]]), (B, 1)), np.tile(np.int32([[20, 20, 21, 22]]), (B, 1))) if self.two else (None, None)
        o = explain_oracle(imp0, imp1, rel0, ent1, rel1, ent2, top, n_relation=3)
        res = {k: torch.from_numpy(o[k]) for k in ("paths", "mass", "slot", "distinct", "total")}
        res["scores"] = torch.full((B,), 0.625)
        res["weight"] = res["mass"].double() / ONE
        if profile:
            res["rel_mass"] = torch.from_numpy(o["rel_mass"])
        return res


def test_explain_pairs_records_and_names():
    ent_names, rel_names = {"10": "Alien", "20": "Ridley Scott", "5": "The item"}, {"1": "directed_by", "0": "born_in"}
    recs = harness.explain_pairs(_StubFeeder(), [3, 4], [5, 6], 3, entity_names=ent_names, relation_names=rel_names)
    assert [r["user"] for r in recs] == [3, 4] and [r["item"] for r in recs] == [5, 6]
    r = recs[0]
    assert r["item_name"] == "The item" and recs[1]["item_name"] == "6" and r["score"] == 0.625
    assert r["distinct"] == 3 and r["total_weight"] == 1.0 and len(r["paths"]) == 3
    p = r["paths"][0]                                          # slots 0 and 1 merge: 0.75 * (0.5 + 0.5)
    assert p["relations"] == [1, 0] and p["entities"] == [10, 20] and p["weight"] == 0.75 and p["share"] == 0.75 and p["slot"] == 0
    assert p["relation_names"] == ["directed_by", "born_in"] and p["entity_names"] == ["Alien", "Ridley Scott"]
    assert r["paths"][1]["entities"] == [11, 21] and r["paths"][1]["weight"] == 0.25 and r["paths"][1]["entity_names"] == ["11", "21"]
    assert r["paths"][2]["mass"] == 0 and r["paths"][2]["slot"] == 3
    # fewer distinct paths than asked for: only those are listed; no tables: the ids as strings
    recs = harness.explain_pairs(_StubFeeder(two=False), [3], [5], 2)
    assert [p["relations"] for p in recs[0]["paths"]] == [[1], [2]] and recs[0]["paths"][0]["entity_names"] == ["10"]
    assert recs[0]["paths"][0]["weight"] == 0.75 and recs[0]["total_weight"] == 1.0


def test_relation_profile_shares():
    f = _StubFeeder()
    data = np.int64([[0, 5, 1], [1, 6, 0], [2, 7, 1]])
    prof = harness.relation_profile(f, data, batch_size=2)
    assert f.calls == [dict(top=1, profile=True, max_pairs=2)] and prof["n_pairs"] == 3
    assert prof["mass"].tolist() == [[0, 3 * (3 * ONE // 4), 3 * (ONE // 4)], [3 * (3 * ONE // 4), 0, 3 * (ONE // 4)]]
    assert prof["share"].tolist() == [[0.0, 0.75, 0.25], [0.75, 0.0, 0.25]]
    prof = harness.relation_profile(_StubFeeder(two=False), data, batch_size=8)
    assert prof["share"][1].tolist() == [0.0, 0.0, 0.0] and prof["share"][0].tolist() == [0.0, 0.75, 0.25]
