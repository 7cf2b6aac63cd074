"""CPU: tests/keyaddr_ref.py itself -- the float64 reference of MVIN._key_addressing against the from-the-equations oracle and by hand, its
two association orders against each other, and every logit regime's condition at every shape tests/test_gpu_keyaddr_sharp.py uses, so that
nobody needs a GPU to find out that an input is not what it claims."""
import numpy as np
import pytest
import torch

import keyaddr_ref as kr
from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

ALL_SHAPES = sorted({tuple(sorted(c.items())) for cases in kr.CASES.values() for c in cases})


def test_reference_equals_the_equations_oracle():
    from oracle import equations_fp64
    for P, ablation in ((2, "all"), (3, "no_ps_o_ft")):
        args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=12, batch_size=23, ablation=ablation)
        case = synth.small_case(args, n_user=9, n_entity=80, n_relation=5, seed=P)
        params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=1, random_agg_bias=True)
        for k in ("entity_emb_matrix", "relation_emb_KGE_matrix", "h_emb_item_mlp_matrix"):       # away from initialisation: logits of order 10
            params[k] = params[k] * 12
        e = equations_fp64.forward(args, params, case.adj_entity, case.adj_relation, case.users, case.items, case.memories_h, case.memories_r,
                                   case.memories_t)
        t = lambda x: torch.from_numpy(np.asarray(x))             # noqa: E731
        w = t(params["h_emb_item_mlp_matrix"])[:16, 0] if args.PS_O_ft else None
        mem = tuple([t(m) for m in lst] for lst in (case.memories_h, case.memories_r, case.memories_t))
        for order in ("rh_v", "vr_h"):
            r = kr.keyaddr_reference(t(params["entity_emb_matrix"]), t(params["relation_emb_KGE_matrix"]), w, t(params["user_mlp_matrix"]),
                                     t(params["user_mlp_bias"]), mem, t(case.users), t(case.items), P, order=order)
            assert r.o.shape == (23, P + (w is not None), 16)
            assert float(max(lg.std() for lg in r.logits)) > 1
            np.testing.assert_allclose(r.user_o.numpy(), e.user_o, rtol=1e-12, atol=1e-13)


def test_reference_by_hand_on_a_two_memory_row():
    E = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, 1.0], [0.5, -1.0]])
    R = torch.tensor([[[1.0, 2.0], [0.0, 1.0]], [[0.0, 1.0], [-1.0, 0.0]]])
    w = torch.tensor([0.5, 0.25])
    mh, mr, mt = [torch.tensor([[1, 2]])], [torch.tensor([[0, 1]])], [torch.tensor([[3, 0]])]
    r = kr.keyaddr_reference(E, R, w, None, None, (mh, mr, mt), torch.tensor([0]), torch.tensor([2]), 1)
    # hop: R[0] . E[1] = (4, 2), . E[2] = 14;  R[1] . E[2] = (1, -3), . E[2] = 0  ->  p = (1, e^-14) / (1 + e^-14)
    q = np.exp(-14.0) / (1 + np.exp(-14.0))
    np.testing.assert_allclose(r.logits[1].numpy(), [[14.0, 0.0]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r.probs[1].numpy(), [[1 - q, q]], rtol=1e-14)
    np.testing.assert_allclose(r.o[0, 1].numpy(), [(1 - q) * 0.5 + q * 1.0, (1 - q) * -1.0], rtol=1e-14)
    # h-set: E[1] . w = 0.5, E[2] . w = 1.75  ->  p = (1, e^1.25) / (1 + e^1.25), over the HEADS
    a = 1 / (1 + np.exp(1.25))
    np.testing.assert_allclose(r.logits[0].numpy(), [[0.5, 1.75]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r.o[0, 0].numpy(), [(1 - a) * 3.0, a * 2.0 + (1 - a) * 1.0], rtol=1e-14)
    assert r.user_o is None


def test_a_one_hot_row_returns_its_tail_exactly():
    inp = kr.build_inputs("planted", 64, 40, 2, 9, 37)
    r = kr.reference(inp)
    _, tails = kr.planted_rows(inp)
    for p in r.probs:
        assert float(p.max(-1).values.min()) == 1.0           # exp(-40) is below half an ulp of 1 in float64
    assert torch.equal(r.o, tails.double())


@pytest.mark.parametrize("regime", kr.REGIMES)
def test_both_association_orders_agree_in_float64(regime):
    inp = kr.build_inputs(regime, 32, 40, 2, 12, 37)
    a, b = kr.reference(inp, order="rh_v"), kr.reference(inp, order="vr_h")
    scale = max(1.0, float(a.o.abs().max()))
    assert float((a.o - b.o).abs().max()) <= 1e-12 * scale
    assert float((a.user_o - b.user_o).abs().max()) <= 1e-12 * max(1.0, float(a.user_o.abs().max()))
    c = kr.reference(inp, order="rh_v", tw=True)
    assert float((a.user_o - c.user_o).abs().max()) <= 1e-12 * max(1.0, float(a.user_o.abs().max()))


@pytest.mark.parametrize("regime", kr.REGIMES)
def test_every_regime_is_what_it_claims_at_every_gpu_shape(regime):
    for key in ALL_SHAPES:
        c = dict(key)
        inp = kr.build_inputs(regime, **c)
        assert inp.users.shape[0] >= max(kr.YARDSTICK_PAIRS, c["n_pairs"])
        kr.condition(inp, kr.reference(inp))


def test_planted_slots_cover_the_tile_edges():
    for Nm, P, n in ((64, 2, 30), (40, 2, 30), (80, 2, 30), (17, 2, 37), (100, 2, 33), (300, 1, 29)):
        seen = {kr.planted_slot(u, j, P, Nm) for u in range(n) for j in range(P)}
        want = {0, Nm - 1} | {b - 1 for b in range(16, Nm, 16) if b <= 64} | {b for b in range(16, Nm, 16) if b <= 64}
        assert want <= seen, (Nm, sorted(want - seen))
    assert {kr.planted_slot(u, j, 2, 64) for u in range(37) for j in range(2)} == set(range(64))      # every slot where users x hops >= Nm
    assert sorted(kr.key_slots(40)) == list(range(40))


@pytest.mark.parametrize("regime", kr.REGIMES)
def test_the_yardstick_is_finite_and_not_zero(regime):
    for c in (kr.CASES["stream"][2], kr.CASES["dense"][0], kr.CASES["flash"][3]):
        inp = kr.build_inputs(regime, **c)
        ref = kr.reference(inp)
        y = kr.yardstick(inp, ref, tw=True)
        for name, v in y.items():
            if regime == "planted" and name == "o":          # a one-hot row in fp32 returns the tail row itself
                assert v == 0.0 or np.isfinite(v)
                continue
            assert np.isfinite(v) and 0 < v < 1e-2 * max(1.0, float(getattr(ref, name).abs().max())), (regime, name, v)
