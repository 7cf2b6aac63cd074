"""CPU: explaining the user side of a score (mvin_explain_memories, ops.explain_memories, DeviceFeeder.explain_memories,
harness.explain_user_memories) where no GPU is needed -- the selection oracle the GPU tests compare against, checked by hand;
the mass against exact rational arithmetic; the additivity identity the feature rests on, in float64 against
oracle.equations_fp64; the ABI's symbols and refusals before any launch; the ValueErrors of the Python layers; the records
of the harness on a stubbed feeder."""
import ctypes as C
import fnmatch
import os
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mvin_amd import harness, ops
from oracle import equations_fp64 as eq
from explain_memories_oracle import arith_oracle, block_names, f32_sum_ascending, rank_oracle

ONE = 1 << 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- oracle (a), by hand
def _five_slots():
    """One user, one hop, Nm = 5: slots 0 + 2 and 1 + 4 carry the same triple (two duplicates), slot 3 is alone; the merged
    (2, 1, 6) and the single (3, 2, 7) tie exactly."""
    uts = np.int32([[[[1, 2, 1, 3, 2], [0, 1, 0, 2, 1], [5, 6, 5, 7, 6]]]])             # [1, 1, 3, 5]
    probs = np.float32([[[0.25, 0.125, 0.25, 0.25, 0.125]]])
    contrib = np.float32([[[0.5, -0.25, 0.25, 1.0, 0.125]]])
    return uts, probs, contrib


def test_oracle_by_hand_hop_block():
    uts, probs, contrib = _five_slots()
    o = rank_oracle(probs, contrib, uts, [0], P=1, has_set=False, top=4, n_relation=3)
    q = ONE // 8
    # (1,0,5) = slots 0 + 2: 0.5.  (2,1,6) = slots 1 + 4 and (3,2,7) = slot 3 TIE at 0.25: the lower slot first.  Then padding
    assert o["mem"][0, 0].tolist() == [[1, 0, 5], [2, 1, 6], [3, 2, 7], [-1, -1, -1]]
    assert o["mass"][0, 0].tolist() == [4 * q, 2 * q, 2 * q, 0] and o["slot"][0, 0].tolist() == [0, 1, 3, -1]
    assert o["contrib"][0, 0].tolist() == [0.75, -0.125, 1.0, 0.0]
    assert o["distinct"][0, 0] == 3 and o["total"][0, 0] == ONE and o["block"][0, 0] == np.float32(1.625)
    assert o["rel_mass"].tolist() == [[4 * q, 2 * q, 2 * q]]
    # a smaller top is a prefix; a user id out of range is clamped for the read
    o1 = rank_oracle(probs, contrib, uts, [7], P=1, has_set=False, top=2)
    assert np.array_equal(o1["mem"], o["mem"][:, :, :2]) and np.array_equal(o1["mass"], o["mass"][:, :, :2]) and o1["rel_mass"] is None
    # a relation id out of [0, n_relation) is compared and reported raw and adds nothing to the profile
    uts[0, 0, 1] = [-4, 1, -4, 9, 1]
    o = rank_oracle(probs, contrib, uts, [0], P=1, has_set=False, top=3, n_relation=3)
    assert o["mem"][0, 0].tolist() == [[1, -4, 5], [2, 1, 6], [3, 9, 7]] and o["rel_mass"].tolist() == [[0, 2 * q, 0]]


def test_oracle_by_hand_h_set_block_and_h_equal_t_different():
    uts, probs, contrib = _five_slots()
    uts[0, 0, 2] = [5, 6, 8, 7, 6]                             # slots 0 and 2: h equal, t different
    o = rank_oracle(np.tile(probs, (1, 2, 1)), np.tile(contrib, (1, 2, 1)), uts, [0], P=1, has_set=True, top=5, n_relation=3)
    q = ONE // 8
    # the h-set block merges on h alone: 1 -> slots 0 + 2, 2 -> slots 1 + 4, 3 -> slot 3
    assert o["mem"][0, 0].tolist() == [[1, -1, -1], [2, -1, -1], [3, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert o["mass"][0, 0].tolist() == [4 * q, 2 * q, 2 * q, 0, 0] and o["distinct"][0, 0] == 3
    # the hop block does not: four memories; three tie at 0.25 and come by slot
    assert o["mem"][0, 1].tolist() == [[1, 0, 5], [2, 1, 6], [1, 0, 8], [3, 2, 7], [-1, -1, -1]]
    assert o["mass"][0, 1].tolist() == [2 * q, 2 * q, 2 * q, 2 * q, 0] and o["slot"][0, 1].tolist() == [0, 1, 2, 3, -1]
    assert o["distinct"][0, 1] == 4 and o["rel_mass"].tolist() == [[4 * q, 2 * q, 2 * q]]
    assert block_names(2, True) == ["h_set", "hop0", "hop1"] and block_names(1, False) == ["hop0"]


def test_contributions_are_summed_in_ascending_slot_order():
    """float32 addition is not associative: the rule fixes the order, and the oracle keeps it."""
    c = np.float32([1.0, 2.0 ** -24, 2.0 ** -24, -1.0])
    assert f32_sum_ascending(c) == np.float32(0.0) and f32_sum_ascending(c[::-1]) == np.float32(2.0 ** -23)
    uts = np.zeros((1, 1, 3, 4), np.int32)                     # all four slots are one memory
    o = rank_oracle(np.full((1, 1, 4), 0.25, np.float32), c.reshape(1, 1, 4), uts, [0], 1, False, 1)
    assert o["contrib"][0, 0, 0] == np.float32(0.0) and o["block"][0, 0] == np.float32(0.0) and o["mass"][0, 0, 0] == ONE


# --------------------------------------------------------------------------- the mass definition
def test_mass_is_exact_rational_arithmetic():
    rng = np.random.default_rng(11)
    p = rng.random((40, 2, 16)).astype(np.float32)
    p[0, 0, :6] = [np.nan, np.inf, -0.5, 0.0, 1.5, 1e-45]
    p[1, 1, :3] = np.float32(2.0) ** np.float32([-41, -40, -39])
    uts = rng.integers(0, 4, (5, 2, 3, 16)).astype(np.int32)
    users = rng.integers(0, 5, 40)
    o = rank_oracle(p, np.zeros_like(p), uts, users, P=2, has_set=False, top=16)

    def exact(w):
        w = float(w)
        if not np.isfinite(w) or w <= 0:
            return 0
        return (Fraction(min(w, 1.0)) * ONE).__floor__()
    for b in range(40):
        for c in range(2):
            assert int(o["total"][b, c]) == sum(exact(w) for w in p[b, c]), (b, c)
            assert int(o["mass"][b, c].sum()) == int(o["total"][b, c])                     # top = Nm lists every memory
    assert exact(np.float32(2.0 ** -41)) == 0 and exact(np.float32(2.0 ** -40)) == 1 and exact(np.float32(1.5)) == ONE


# --------------------------------------------------------------------------- the additivity identity, float64
@pytest.mark.parametrize("P,ft", [(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_parts_add_up_to_the_score_in_float64(P, ft):
    """sum_c block_c + bias . v' == pair_user_vector(...) . v' for any v': the score is additive over the memories."""
    rng = np.random.default_rng(100 + 10 * P + ft)
    D, Nm, nE, nR, nU, B = 8, 6, 30, 4, 5, 7
    n_o = P + ft
    args = SimpleNamespace(dim=D, PS_O_ft=ft, p_hop=P)
    p = dict(entity_emb_matrix=rng.normal(size=(nE, D)), user_emb_matrix=rng.normal(size=(nU, D)),
             relation_emb_KGE_matrix=rng.normal(size=(nR, D, D)), h_emb_item_mlp_matrix=rng.normal(size=(2 * D, 1)),
             h_emb_item_mlp_bias=rng.normal(size=(1,)), user_mlp_matrix=rng.normal(size=(n_o * D, D)),
             user_mlp_bias=rng.normal(size=(D,)))
    uts = np.stack([rng.integers(0, nE, (nU, max(1, P), Nm)), rng.integers(0, nR, (nU, max(1, P), Nm)),
                    rng.integers(0, nE, (nU, max(1, P), Nm))], axis=2).astype(np.int32)
    uts[:, :, :, Nm - 2:] = uts[:, :, :, :2]                   # repeated memories, as the sampler draws them
    users, items = rng.integers(0, nU, B), rng.integers(0, nE, B)
    v_final = rng.normal(size=(B, D))                          # the final item embedding: E[item] under PS_only, anything else otherwise
    E = p["entity_emb_matrix"]
    V = np.einsum("bd,rde->bre", E[items], p["relation_emb_KGE_matrix"]) if P else None
    G = v_final @ p["user_mlp_matrix"].T
    o = arith_oracle(E, V, p["h_emb_item_mlp_matrix"][:D, 0] if ft else None, uts, users, G, p["user_mlp_bias"], v_final, P)
    parts = o["block"].sum(axis=1) + o["bias"]
    for b in range(B):
        sel = uts[users[b]]
        user_o = eq.pair_user_vector(args, p, int(users[b]), int(items[b]), sel[:, 0], sel[:, 1], sel[:, 2])
        want = float(user_o @ v_final[b])
        assert abs(parts[b] - want) <= 1e-12 * max(1.0, abs(want)), (b, parts[b], want)
        assert np.allclose(o["probs"][b].sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    # and the ranked contributions of a block add up to it when every memory is listed
    r = rank_oracle(o["probs"].astype(np.float32), o["slot_contrib"].astype(np.float32), uts, users, P, bool(ft), Nm)
    assert np.allclose(r["contrib"].astype(np.float64).sum(axis=2), o["block"], rtol=0, atol=1e-5 * np.abs(o["value"]).max())
    assert (r["distinct"] <= Nm - 1).all()


# --------------------------------------------------------------------------- the C ABI
NAMES = ("mvin_explain_memories", "mvin_explain_memories_max_nm")


def _p(x):
    return None if x is None else C.c_void_p(x)


_PTRS = ("entity_emb", "V", "w_h", "uts", "users", "G", "mlp_bias", "item_final")
_OUTS = ("out_mem", "out_mass", "out_contrib", "out_slot", "out_distinct", "out_total", "out_block", "out_bias", "out_probs",
         "out_slot_contrib", "rel_mass")


def _call(lib, B=4, P=2, Nm=16, D=8, nR=5, n_entity=30, n_user=6, top=3, **ptr):
    for k in _PTRS + _OUTS[:8]:
        ptr.setdefault(k, 16)                                  # fake device addresses: never dereferenced before a launch
    for k in _OUTS[8:]:
        ptr.setdefault(k, None)
    return lib.mvin_explain_memories(*[_p(ptr[k]) for k in _PTRS], B, P, Nm, D, nR, n_entity, n_user, top,
                                     *[_p(ptr[k]) for k in _OUTS], None)


def test_symbols_in_header_map_and_library(hip_lib):
    from mvin_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    vmap = open(os.path.join(ROOT, "mvin_amd", "csrc", "libmvin_hip.map")).read()
    exported = re.search(r"global:\s*([^;]+);", vmap).group(1).split()
    for name in NAMES:
        assert re.search(r"MVIN_API int %s\(" % name, header), name
        assert name in vmap and any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None
    assert len(_lib.SIGNATURES["mvin_explain_memories"][1]) == 28
    assert hip_lib.mvin_explain_memories_max_nm() == 64 == ops.explain_memories_max_nm()
    assert hip_lib.mvin_abi_version() == 12                    # entry points were only added


def test_abi_validates_before_launching(hip_lib):
    # every failing call fails on the host: the fake device pointers are never dereferenced and nothing is launched
    null = [{k: None} for k in _PTRS if k != "w_h"] + [{k: None} for k in _OUTS[:8]]
    size = [dict(Nm=65), dict(Nm=0), dict(D=6), dict(D=0), dict(D=132), dict(top=0), dict(top=17), dict(Nm=5, top=6), dict(P=9),
            dict(P=-1), dict(P=0, w_h=None), dict(B=-1), dict(B=(1 << 31) // (3 * 16) + 1), dict(n_entity=0), dict(n_user=0), dict(nR=0),
            dict(rel_mass=16, B=(1 << 18) + 1), dict(rel_mass=16, P=0)]
    for code, cases in ((-1, null), (-2, size)):
        for kw in cases:
            assert _call(hip_lib, **kw) == code, kw
            assert b"mvin_explain_memories" in hip_lib.mvin_last_error(), kw
    # B == 0 is valid and launches nothing, at the limits of every size; V may be NULL when there is no hop block
    assert _call(hip_lib, B=0) == 0 and _call(hip_lib, B=0, Nm=64, top=64, D=128, P=8) == 0
    assert _call(hip_lib, B=0, Nm=1, top=1, D=4, P=0, V=None) == 0 and _call(hip_lib, B=0, w_h=None) == 0
    assert _call(hip_lib, B=0, rel_mass=16, out_probs=16, out_slot_contrib=16) == 0


# --------------------------------------------------------------------------- ops.explain_memories
def _op_args(B=3, P=1, Nm=4, D=8, nR=5, nE=20, nU=6, n_o=2, table=torch.float32):
    return dict(entity_emb=torch.zeros((nE, D), dtype=table), V=torch.zeros((B, nR, D)), w_h=torch.zeros(2 * D) if n_o > P else None,
                uts=torch.zeros((nU, max(1, P), 3, Nm), dtype=torch.int32), users=torch.zeros(B, dtype=torch.int64),
                G=torch.zeros((B, n_o * D)), mlp_bias=torch.zeros(D), item_final=torch.zeros((B, D)), P=P, top=2)


def test_ops_refuse_bad_shapes_and_cpu_tensors(hip_lib):
    from mvin_amd import _lib
    bad = [(dict(table=torch.bfloat16), {}, "fp32"), (dict(Nm=65), {}, "Nm=65"), (dict(D=6), {}, "D=6"), ({}, dict(top=0), "top=0"),
           ({}, dict(top=5), "top=5"), (dict(P=0, n_o=0), {}, "at least one block"), ({}, dict(P=2), "uts"),
           ({}, dict(G=torch.zeros((3, 8))), "G"), ({}, dict(V=None), "V"), ({}, dict(V=torch.zeros((2, 5, 8))), "V"),
           ({}, dict(item_final=torch.zeros((3, 4))), "item_final"), ({}, dict(rel_mass=torch.zeros((2, 5), dtype=torch.int64)), "rel_mass")]
    for shape, over, match in bad:
        kw = _op_args(**shape)
        kw.update(over)
        with pytest.raises(ValueError, match=match):
            ops.explain_memories(**kw)
    with pytest.raises(_lib.MvinHipError):                     # the shapes are right: what is left is that there is no CPU path
        ops.explain_memories(**_op_args())


# --------------------------------------------------------------------------- the feeder's refusals, on a stubbed model
def _stub_feeder(**kw):
    args = dict(HO_only=0, PS_O_ft=1)
    args.update({k: kw.pop(k) for k in list(kw) if k in args})
    model = dict(table_dtype="f32", p_hop=2, n_memory=16, dim=8, n_relation=5, device="cpu")
    model.update(kw)
    f = object.__new__(harness.DeviceFeeder)
    f.model = SimpleNamespace(args=SimpleNamespace(**args), **model)
    return f


def test_feeder_refuses_what_it_cannot_explain(hip_lib):
    with pytest.raises(ValueError, match="HO_only"):
        _stub_feeder(HO_only=1).explain_memories([0], [1])
    with pytest.raises(ValueError, match="bf16"):
        _stub_feeder(table_dtype="bf16").explain_memories([0], [1])
    with pytest.raises(ValueError, match="n_memory=65"):
        _stub_feeder(n_memory=65).explain_memories([0], [1])
    with pytest.raises(ValueError, match="no ripple set"):
        _stub_feeder(p_hop=0, PS_O_ft=0).explain_memories([0], [1])
    for kw in (dict(top=0), dict(top=17), dict(max_pairs=0)):
        with pytest.raises(ValueError, match="top"):
            _stub_feeder().explain_memories([0], [1], **kw)
    with pytest.raises(ValueError, match="2 users for 1 items"):
        _stub_feeder().explain_memories([0, 1], [1])


# --------------------------------------------------------------------------- the harness on a stubbed feeder
class _StubFeeder(object):
    """DeviceFeeder.explain_memories replaced by the oracle on hand-made attention: what explain_user_memories does with it."""
    def __init__(self):
        self.model = SimpleNamespace(args=SimpleNamespace(PS_O_ft=1))
        self.calls = []

    def explain_memories(self, users, items, top=10, profile=False, return_attention=False, max_pairs=4096):
        self.calls.append(dict(top=top, profile=profile, max_pairs=max_pairs))
        B = len(users)
        uts, probs, contrib = _five_slots()
        o = rank_oracle(np.tile(probs, (B, 2, 1)), np.tile(contrib, (B, 2, 1)), uts, np.zeros(B, np.int64), 1, True, top, n_relation=3)
        res = {k: torch.from_numpy(o[k]) for k in ("mem", "mass", "contrib", "slot", "distinct", "total", "block")}
        res["bias"] = torch.full((B,), 0.75)
        res["score_parts"] = torch.cat([res["block"], res["bias"][:, None]], dim=1)
        res["scores"] = res["score_parts"].sum(dim=1)          # 1.625 + 1.625 + 0.75 = 4.0
        res["scores_normalized"] = torch.sigmoid(res["scores"])
        res["weight"] = res["mass"].double() / ONE
        if profile:
            res["rel_mass"] = torch.from_numpy(o["rel_mass"])
        return res


def test_explain_user_memories_records_and_shares():
    ent_names, rel_names = {"1": "Alien", "5": "Ridley Scott", "9": "The item"}, {"0": "directed_by"}
    f = _StubFeeder()
    recs = harness.explain_user_memories(f, [3, 4], [9, 6], 3, entity_names=ent_names, relation_names=rel_names)
    assert f.calls == [dict(top=3, profile=False, max_pairs=4096)]
    assert [r["user"] for r in recs] == [3, 4] and [r["item"] for r in recs] == [9, 6]
    r = recs[0]
    assert r["item_name"] == "The item" and recs[1]["item_name"] == "6" and r["score"] == 4.0 and r["bias"] == 0.75
    assert r["score_normalized"] == float(torch.sigmoid(torch.tensor(4.0)))
    assert [b["block"] for b in r["blocks"]] == ["h_set", "hop0"]
    hs, hop = r["blocks"]
    assert hs["contribution"] == 1.625 and hs["distinct"] == 3 and hs["total_weight"] == 1.0 and len(hs["memories"]) == 3
    m = hs["memories"][0]
    assert (m["block"], m["h"], m["r"], m["t"]) == ("h_set", 1, None, None) and m["h_name"] == "Alien" and m["r_name"] is None
    assert m["weight"] == 0.5 and m["contribution"] == 0.75 and m["share"] == 0.75 / 4.0 and m["slot"] == 0 and m["mass"] == ONE // 2
    m = hop["memories"][0]
    assert (m["block"], m["h"], m["r"], m["t"]) == ("hop0", 1, 0, 5)
    assert (m["h_name"], m["r_name"], m["t_name"]) == ("Alien", "directed_by", "Ridley Scott")
    m = hop["memories"][1]                                     # the tie: the lower slot first; a negative contribution keeps its sign
    assert (m["h"], m["r"], m["t"], m["slot"]) == (2, 1, 6, 1) and m["contribution"] == -0.125 and m["share"] == -0.125 / 4.0
    assert (m["h_name"], m["r_name"], m["t_name"]) == ("2", "1", "6")
    # the shares of everything listed plus the bias are the score when every memory is listed
    recs = harness.explain_user_memories(_StubFeeder(), [3], [9], 5)
    tot = sum(m["share"] for b in recs[0]["blocks"] for m in b["memories"]) + recs[0]["bias"] / recs[0]["score"]
    assert tot == 1.0 and [len(b["memories"]) for b in recs[0]["blocks"]] == [3, 3]


def test_memory_relation_profile_shares():
    f = _StubFeeder()
    data = np.int64([[0, 5, 1], [1, 6, 0], [2, 7, 1]])
    prof = harness.memory_relation_profile(f, data, batch_size=2)
    assert f.calls == [dict(top=1, profile=True, max_pairs=2)] and prof["n_pairs"] == 3
    assert prof["mass"].tolist() == [[3 * (ONE // 2), 3 * (ONE // 4), 3 * (ONE // 4)]]
    assert prof["share"].tolist() == [[0.5, 0.25, 0.25]]
