"""-m gpu: DeviceFeeder.explain, harness.explain_pairs and harness.relation_profile end to end -- the paths of a real forward
pass against the oracle applied to the attention tensors the pass returned and to get_neighbors' ids, on an adjacency with
repeated slots (rows as the reference's sampler builds them for low-degree entities)."""
import numpy as np
import pytest
import torch

from mvin_amd import harness, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from explain_oracle import explain_oracle
from parity import ATOL, RTOL, assert_close

pytestmark = pytest.mark.gpu

ONE = 1 << 40
SHAPES = {"d16k8": dict(dim=16, neighbor_sample_size=8), "d64k32": dict(dim=64, neighbor_sample_size=32)}
_built = {}


def build(name, **kw):
    """The build() shape of tests/test_gpu_api.py (24 pairs, 20 users, 300 entities, 6 relations) with repeated slots."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _built:
        from mvin_amd.model import MVIN
        d = dict(h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=24)
        d.update(SHAPES[name])
        d.update(kw)
        args = make_args(**d)
        case = synth.small_case(args, n_user=20, n_entity=300, n_relation=6, seed=31, zero_rows=4, repeats=True)
        params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=32, random_agg_bias=True)
        model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params,
                     device="cuda:0")
        uts = synth.ripple_sets(case.n_user, case.n_entity, case.n_relation, args.p_hop, args.n_memory, seed=33)
        _built[key] = (args, case, model, harness.DeviceFeeder(model, uts))
    return _built[key]


def oracle_of(model, res, items, top, two=True):
    """The oracle on the attention tensors ``explain`` returned and on get_neighbors' ids of the same items."""
    it = torch.from_numpy(np.asarray(items, np.int64)).to(model.device)
    ents, rels = model.get_neighbors(it, levels=2 if two else 1)
    cpu = lambda t: t.cpu().numpy()
    return explain_oracle(cpu(res["imp0"]), cpu(res["imp1"]) if two else None, cpu(rels[0]), cpu(ents[1]),
                          cpu(rels[1]) if two else None, cpu(ents[2]) if two else None, top, n_relation=model.n_relation)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_explain_equals_oracle_on_its_attention(hip_lib, name):
    args, case, model, feeder = build(name)
    K = args.neighbor_sample_size
    B, top = len(case.users), 10
    res = feeder.explain(case.users, case.items, top=top, profile=True, return_attention=True)
    assert res["imp0"].shape == (B, 1, K) and res["imp1"].shape == (B, K, K)
    want = oracle_of(model, res, case.items, top)
    for n in ("paths", "mass", "slot", "distinct", "total", "rel_mass"):
        got = res[n].cpu().numpy()
        assert got.dtype == want[n].dtype and np.array_equal(got, want[n]), n
    assert res["weight"].dtype == torch.float64 and np.array_equal(res["weight"].cpu().numpy(), want["mass"] / float(ONE))
    # repeated slots merge: far fewer distinct paths than slots, somewhere at least
    assert want["distinct"].min() < K * K and (want["distinct"] >= 1).all()
    # the scores are the model's: the want_probs pass takes another kernel form, so to rounding
    assert_close(res["scores"].cpu().numpy(), feeder.scores(case.users, case.items).cpu().numpy(), "scores", rtol=RTOL, atol=ATOL)
    # both softmaxes sum to 1 in float32 and a mass loses less than 2^-40 to its floor: all weights of a pair sum to 1
    total = res["total"].cpu().numpy() / float(ONE)
    print("max |sum of weights - 1| =", np.abs(total - 1).max(), "bound", K * K * 2.0 ** -23)
    assert np.abs(total - 1).max() <= K * K * 2.0 ** -23
    # in chunks (one pass per 7 pairs; the last holds 3): every chunk lands in its rows, the profile is summed over them
    again = feeder.explain(case.users, case.items, top=top, profile=True, return_attention=True, max_pairs=7)
    want = oracle_of(model, again, case.items, top)
    for n in ("paths", "mass", "slot", "distinct", "total", "rel_mass"):
        assert np.array_equal(again[n].cpu().numpy(), want[n]), n
    assert_close(again["scores"].cpu().numpy(), res["scores"].cpu().numpy(), "scores in chunks", rtol=RTOL, atol=ATOL)


def test_one_hop_model_takes_one_hop_mode(hip_lib):
    args, case, model, feeder = build("d16k8", h_hop=1)
    K = args.neighbor_sample_size
    res = feeder.explain(case.users, case.items, top=K, profile=True, return_attention=True)
    assert res["imp1"] is None and res["imp0"].shape == (len(case.users), 1, K)
    want = oracle_of(model, res, case.items, K, two=False)
    for n in ("paths", "mass", "slot", "distinct", "total", "rel_mass"):
        assert np.array_equal(res[n].cpu().numpy(), want[n]), n
    assert (res["paths"][:, :, 2:] == -1).all() and (want["rel_mass"][1] == 0).all()
    with pytest.raises(ValueError, match="top"):
        feeder.explain(case.users, case.items, top=K + 1)


def test_model_without_attention_is_refused(hip_lib):
    args, case, model, feeder = build("d16k8", User_orient_rela=0)
    with pytest.raises(ValueError, match="no attention outputs"):
        feeder.explain(case.users, case.items, top=3)


def test_explain_pairs_returns_named_records(hip_lib):
    args, case, model, feeder = build("d16k8")
    ent_names = {str(i): f"entity<{i}>" for i in range(0, case.n_entity, 2)}                 # every other entity has a name
    rel_names = {str(i): f"rel<{i}>" for i in range(case.n_relation)}
    top = 4
    recs = harness.explain_pairs(feeder, case.users, case.items, top, entity_names=ent_names, relation_names=rel_names)
    res = feeder.explain(case.users, case.items, top=top)
    paths, mass, total = res["paths"].cpu().numpy(), res["mass"].cpu().numpy(), res["total"].cpu().numpy()
    scores, distinct = res["scores"].cpu().numpy(), res["distinct"].cpu().numpy()
    assert len(recs) == len(case.users)
    for b, r in enumerate(recs):
        assert (r["user"], r["item"], r["distinct"]) == (case.users[b], case.items[b], distinct[b])
        assert r["score"] == float(scores[b]) and r["total_weight"] == total[b] / float(ONE)
        assert r["item_name"] == ent_names.get(str(case.items[b]), str(case.items[b]))
        assert len(r["paths"]) == min(top, distinct[b])
        for p, rec in enumerate(r["paths"]):
            assert rec["relations"] == [paths[b, p, 0], paths[b, p, 2]] and rec["entities"] == [paths[b, p, 1], paths[b, p, 3]]
            assert rec["relation_names"] == [f"rel<{i}>" for i in rec["relations"]]
            assert rec["entity_names"] == [ent_names.get(str(i), str(i)) for i in rec["entities"]]
            assert rec["mass"] == mass[b, p] and rec["weight"] == mass[b, p] / float(ONE) and rec["share"] == mass[b, p] / total[b]
        assert [rec["mass"] for rec in r["paths"]] == sorted((rec["mass"] for rec in r["paths"]), reverse=True)


def test_relation_profile_over_a_split(hip_lib):
    args, case, model, feeder = build("d16k8")
    rng = np.random.default_rng(9)
    data = np.stack([rng.integers(0, case.n_user, 64), rng.integers(0, case.n_entity, 64), rng.integers(0, 2, 64)], axis=1)
    prof = harness.relation_profile(feeder, data, batch_size=24)
    # the oracle on the attention of the same batches (24 + 24 + 16 pairs)
    res = feeder.explain(data[:, 0], data[:, 1], top=1, return_attention=True, max_pairs=24)
    want = oracle_of(model, res, data[:, 1], 1)["rel_mass"]
    assert prof["n_pairs"] == 64 and prof["mass"].dtype == np.int64 and np.array_equal(prof["mass"], want)
    share = want / want.sum(axis=1, keepdims=True)
    assert np.array_equal(prof["share"], share) and np.allclose(prof["share"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
