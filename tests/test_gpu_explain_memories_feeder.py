"""-m gpu: DeviceFeeder.explain_memories, harness.explain_user_memories and harness.memory_relation_profile end to end on real
MVIN models (dim 16 / fan-out 8 / P 2 / Nm 16 and dim 64 / fan-out 32 / P 2 / Nm 64, 64 pairs each; repeated adjacency slots and
ripple sets drawn with repeats).

The parts of a score must ADD UP to it.  ``score_parts.sum(1)`` is one more float32 evaluation of the pair's logit, so it is
held to the rule of the other float32 evaluations here: its error against oracle.equations_fp64.forward may be at most 4 x the
error of the float32 yardstick (oracle.mirror_fp32.forward: the same equations in float32), measured as a maximum over this
module's own inputs, with a floor of 2^-23 in the logit's unit max(1, |logit|).  ``forward_users(...).scores`` is held to the
same bound, so the two float32 evaluations may differ by the sum of their two bounds."""
import numpy as np
import pytest
import torch

from mvin_amd import harness, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from explain_memories_oracle import block_names, rank_oracle
from parity import ATOL, RTOL, assert_close

pytestmark = pytest.mark.gpu

ONE = 1 << 40
FLOOR = 2.0 ** -23
SHAPES = {"d16k8": dict(dim=16, neighbor_sample_size=8, n_memory=16), "d64k32": dict(dim=64, neighbor_sample_size=32, n_memory=64)}
VARIANTS = [("d16k8", {}), ("d64k32", {}), ("d16k8", dict(ablation="ps_only")), ("d16k8", dict(ablation="no_ps_o_ft"))]
_built = {}


def build(name, **kw):
    """Case, parameters and the two CPU oracles' logits; made once per variant, never modified.  The model is built by
    ``model_of`` inside a test, where the suite's kernel pins are in force."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _built:
        d = dict(h_hop=2, n_mix_hop=1, p_hop=2, batch_size=64)
        d.update(SHAPES[name])
        d.update(kw)
        args = make_args(**d)
        case = synth.small_case(args, n_user=20, n_entity=300, n_relation=6, seed=41, zero_rows=4, repeats=True)
        params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=42, random_agg_bias=True)
        uts = synth.ripple_sets(case.n_user, case.n_entity, case.n_relation, args.p_hop, args.n_memory, seed=43)
        uts[:, :, :, args.n_memory // 2:] = uts[:, :, :, :args.n_memory // 4].repeat(2, axis=3)     # a short history, drawn with replacement
        case.memories_h, case.memories_r, case.memories_t = synth.memories_for(uts, case.users)
        from oracle import equations_fp64, mirror_fp32
        feed = (args, params, case.adj_entity, case.adj_relation, case.users, case.items, case.memories_h, case.memories_r,
                case.memories_t)
        ref = equations_fp64.forward(*feed).scores
        mirror = np.asarray(mirror_fp32.forward(*feed).scores, dtype=np.float64)
        _built[key] = SimpleCase(args=args, case=case, params=params, uts=uts, ref=ref, model=None, feeder=None,
                                 yard=float((np.abs(mirror - ref) / np.maximum(1.0, np.abs(ref))).max()))
    return _built[key]


def model_of(name, **kw):
    s = build(name, **kw)
    if s.model is None:
        from mvin_amd.model import MVIN
        case = s.case
        s.model = MVIN(s.args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=s.params,
                       device="cuda:0")
        s.feeder = harness.DeviceFeeder(s.model, s.uts)
    return s


class SimpleCase(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def yardstick():
    """The float32 yardstick's largest logit error over every model of this module, in the logit's unit; computed once."""
    y = max(build(name, **kw).yard for name, kw in VARIANTS)
    print(f"float32 yardstick (mirror_fp32 vs equations_fp64), logit: {y:.3e}")
    return y


@pytest.mark.parametrize("name,kw", VARIANTS, ids=lambda v: v if isinstance(v, str) else (v.get("ablation") or "all"))
def test_parts_add_up_to_the_score(hip_lib, yardstick, name, kw):
    s = model_of(name, **kw)
    args, case, feeder = s.args, s.case, s.feeder
    P, Nm, ft = args.p_hop, args.n_memory, bool(args.PS_O_ft)
    n_o, B = P + int(ft), len(case.users)
    res = feeder.explain_memories(case.users, case.items, top=Nm, profile=True, return_attention=True)
    cpu = {k: v.cpu().numpy() for k, v in res.items()}
    assert cpu["score_parts"].shape == (B, n_o + 1) and cpu["mem"].shape == (B, n_o, Nm, 3) and cpu["probs"].shape == (B, n_o, Nm)
    assert np.array_equal(cpu["score_parts"][:, :n_o], cpu["block"]) and np.array_equal(cpu["score_parts"][:, n_o], cpu["bias"])
    unit = np.maximum(1.0, np.abs(s.ref))
    bound = max(4.0 * yardstick, FLOOR)
    parts = res["score_parts"].sum(dim=1).cpu().numpy().astype(np.float64)
    e_parts = (np.abs(parts - s.ref) / unit).max()
    e_fwd = (np.abs(cpu["scores"].astype(np.float64) - s.ref) / unit).max()
    e_both = (np.abs(parts - cpu["scores"]) / unit).max()
    print(f"{name} {kw}: sum of parts vs float64 {e_parts:.3e}, forward vs float64 {e_fwd:.3e}, parts vs forward {e_both:.3e}  "
          f"(yardstick {yardstick:.3e}, bound {bound:.3e})")
    assert e_parts <= bound, f"sum of parts: error {e_parts:.3e}, float32 yardstick {yardstick:.3e}"
    assert e_both <= 2 * bound, f"sum of parts vs forward_users: {e_both:.3e}, the two bounds add up to {2 * bound:.3e}"
    # the scores are the model's
    assert_close(cpu["scores_normalized"], feeder.scores(case.users, case.items).cpu().numpy(), "sigmoid scores", rtol=RTOL, atol=ATOL)
    assert_close(cpu["scores_normalized"], 1.0 / (1.0 + np.exp(-cpu["scores"].astype(np.float64))), "sigmoid of the logit", rtol=RTOL, atol=ATOL)
    # the ranked outputs are oracle (a) on the attention returned; repeats merged
    want = rank_oracle(cpu["probs"], cpu["slot_contrib"], s.uts, case.users, P, ft, Nm, n_relation=case.n_relation)
    for n in ("mem", "mass", "contrib", "slot", "distinct", "total", "block", "rel_mass"):
        assert cpu[n].dtype == want[n].dtype and np.array_equal(cpu[n].view(np.uint32) if cpu[n].dtype == np.float32 else cpu[n],
                                                               want[n].view(np.uint32) if want[n].dtype == np.float32 else want[n]), n
    assert want["distinct"].max() <= Nm - Nm // 4 and res["weight"].dtype == torch.float64
    assert np.array_equal(cpu["weight"], want["mass"] / float(ONE))
    # a mass loses less than 2^-40 to its floor; p_m = e_m / S with S a float32 tree sum over the 64 lanes (6 levels, 2^-24 each)
    # and one more rounding for the division and for each e_m: sum_m p_m = 1 to within 8 * 2^-24
    total = cpu["total"] / float(ONE)
    weights_bound = Nm * 2.0 ** -40 + 8 * 2.0 ** -24
    print("max |sum of weights - 1| =", np.abs(total - 1).max(), "bound", weights_bound)
    assert np.abs(total - 1).max() <= weights_bound
    # under PS_only the final item embedding is the table's row
    if args.PS_only:
        E = s.model.entity_emb_matrix.float().cpu().numpy()
        assert np.array_equal(s.model.forward_users(*ids(s), feeder.uts).item_embeddings.cpu().numpy(), E[case.items])
    assert block_names(P, ft) == (["h_set"] if ft else []) + ["hop0", "hop1"] and (not ft) == (kw.get("ablation") == "no_ps_o_ft")
    # in chunks (7 pairs per pass; the last holds 1): the same bits, the profile summed over the chunks
    again = feeder.explain_memories(case.users, case.items, top=Nm, profile=True, return_attention=True, max_pairs=7)
    for n in res:
        a, b = again[n].cpu().numpy(), cpu[n]
        if n in ("scores", "scores_normalized"):               # the forward pass of 7 pairs may take another kernel form
            assert_close(a, b, n + " in chunks", rtol=RTOL, atol=ATOL)
        else:
            assert a.tobytes() == b.tobytes(), n


def ids(s):
    dev = s.model.device
    return torch.from_numpy(s.case.users).to(dev), torch.from_numpy(s.case.items).to(dev)


def test_records_and_profile_end_to_end(hip_lib):
    s = model_of("d16k8")
    case, feeder = s.case, s.feeder
    ent_names = {str(i): f"entity<{i}>" for i in range(0, case.n_entity, 2)}
    rel_names = {str(i): f"rel<{i}>" for i in range(case.n_relation)}
    top = 4
    recs = harness.explain_user_memories(feeder, case.users, case.items, top, entity_names=ent_names, relation_names=rel_names)
    res = {k: v.cpu().numpy() for k, v in feeder.explain_memories(case.users, case.items, top=top).items()}
    assert len(recs) == len(case.users)
    for b, r in enumerate(recs):
        assert (r["user"], r["item"]) == (case.users[b], case.items[b]) and r["score"] == float(res["scores"][b])
        assert r["bias"] == float(res["bias"][b]) and [blk["block"] for blk in r["blocks"]] == ["h_set", "hop0", "hop1"]
        for c, blk in enumerate(r["blocks"]):
            assert blk["contribution"] == float(res["block"][b, c]) and blk["distinct"] == res["distinct"][b, c]
            assert len(blk["memories"]) == min(top, res["distinct"][b, c])
            for p, m in enumerate(blk["memories"]):
                h, rr, t = (int(x) for x in res["mem"][b, c, p])
                assert (m["h"], m["r"], m["t"]) == ((h, None, None) if c == 0 else (h, rr, t))
                assert m["h_name"] == ent_names.get(str(h), str(h)) and (c == 0 or m["r_name"] == f"rel<{rr}>")
                assert m["mass"] == res["mass"][b, c, p] and m["weight"] == res["mass"][b, c, p] / float(ONE)
                assert m["contribution"] == float(res["contrib"][b, c, p]) and m["share"] == float(res["contrib"][b, c, p]) / r["score"]
            assert [m["mass"] for m in blk["memories"]] == sorted((m["mass"] for m in blk["memories"]), reverse=True)
    rng = np.random.default_rng(9)
    data = np.stack([rng.integers(0, case.n_user, 64), rng.integers(0, case.n_entity, 64), rng.integers(0, 2, 64)], axis=1)
    prof = harness.memory_relation_profile(feeder, data, batch_size=24)
    att = feeder.explain_memories(data[:, 0], data[:, 1], top=1, return_attention=True, max_pairs=24)
    want = rank_oracle(att["probs"].cpu().numpy(), att["slot_contrib"].cpu().numpy(), s.uts, data[:, 0], 2, True, 1,
                       n_relation=case.n_relation)["rel_mass"]
    assert prof["n_pairs"] == 64 and prof["mass"].dtype == np.int64 and np.array_equal(prof["mass"], want)
    assert np.array_equal(prof["share"], want / want.sum(axis=1, keepdims=True))


def test_item_side_explain_is_unchanged(hip_lib):
    """DeviceFeeder.explain on the same model gives the same bytes before and after explain_memories."""
    s = model_of("d16k8")
    run = lambda: {k: v.cpu().numpy() for k, v in s.feeder.explain(s.case.users, s.case.items, top=5, profile=True).items()}
    before = run()
    s.feeder.explain_memories(s.case.users, s.case.items, top=3, profile=True)
    after = run()
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


def test_refusals_on_real_models(hip_lib):
    s = model_of("d16k8", ablation="ho_only")
    with pytest.raises(ValueError, match="HO_only"):
        s.feeder.explain_memories(s.case.users, s.case.items)
    s = model_of("d16k8")
    with pytest.raises(ValueError, match="top"):
        s.feeder.explain_memories(s.case.users, s.case.items, top=17)
