"""CPU: the training-step oracle (oracle/train_ref.py): loss pieces against a direct numpy
evaluation of model.py:378-412, autograd gradients against central finite differences."""
import numpy as np
import torch

from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from oracle import equations_fp64, train_ref


def setup(**kw):
    d = dict(dim=8, neighbor_sample_size=3, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=4, batch_size=5,
             l2_weight=1e-2, l2_agg_weight=1e-3, lr=1e-2)
    d.update(kw)
    args = make_args(**d)
    case = synth.small_case(args, n_user=6, n_entity=40, n_relation=4, seed=61)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=62, random_agg_bias=True)
    labels = (np.arange(args.batch_size) % 2).astype(np.float32)
    return args, case, params, labels


def test_loss_pieces_match_direct_evaluation():
    args, case, params, labels = setup()
    loss, grads, pieces, out = train_ref.loss_and_grads(args, params, case.adj_entity, case.adj_relation, case.users,
                                                        case.items, labels, case.memories_h, case.memories_r,
                                                        case.memories_t)
    s = equations_fp64.forward(args, params, case.adj_entity, case.adj_relation, case.users, case.items,
                               case.memories_h, case.memories_r, case.memories_t).scores
    base = np.mean(np.maximum(s, 0) - s * labels + np.log1p(np.exp(-np.abs(s))))      # tf sigmoid CE
    assert abs(pieces["base"] - base) < 1e-6
    E, RK = params["entity_emb_matrix"].astype(np.float64), params["relation_emb_KGE_matrix"].astype(np.float64)
    l2 = 0.0
    for hop in range(args.p_hop):
        l2 += (E[case.memories_h[hop]] ** 2).sum() + (E[case.memories_t[hop]] ** 2).sum() + (RK[case.memories_r[hop]] ** 2).sum()
    half = lambda k: (params[k].astype(np.float64) ** 2).sum() / 2
    l2 += half("relation_emb_matrix") + half("user_mlp_matrix") + half("user_mlp_bias")
    l2 += half("transfer_matrix_2") + half("transfer_bias_2")                         # the LAST matrix (:405)
    l2 += sum(half(f"transfer_matrix_{n}") + half(f"transfer_bias_{n}") for n in range(3))   # :407-408
    l2 += half("h_emb_item_mlp_matrix") + half("h_emb_item_mlp_bias")
    assert abs(pieces["l2"] - l2) < 1e-4 * l2
    l2agg = half("user_emb_matrix") + half("enti_transfer_matrix_0") + half("enti_transfer_bias_0")
    l2agg += sum(half(f"agg_{i}_0_weights") + half(f"agg_{i}_0_urh_weights") for i in range(2))
    assert abs(pieces["l2agg"] - l2agg) < 1e-4 * l2agg
    assert abs(loss - (base + args.l2_weight * l2 + args.l2_agg_weight * l2agg)) < 1e-5
    assert "agg_0_0_urh_bias" not in grads            # never used: no gradient (TF skips it)


def test_gradients_match_finite_differences():
    args, case, params, labels = setup(l2_weight=1e-3)
    feed = (case.adj_entity, case.adj_relation, case.users, case.items, labels, case.memories_h, case.memories_r,
            case.memories_t)
    _, grads, _, _ = train_ref.loss_and_grads(args, params, *feed)

    def loss64(p64):
        return train_ref.loss_and_grads(args, p64, *feed, dtype=torch.float64)[0]

    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    rng = np.random.default_rng(0)
    for name in ("entity_emb_matrix", "relation_emb_matrix", "relation_emb_KGE_matrix", "user_emb_matrix",
                 "agg_0_0_urh_weights", "agg_1_0_weights", "transfer_matrix_2", "enti_transfer_matrix_0",
                 "user_mlp_matrix", "h_emb_item_mlp_matrix", "transfer_bias_1", "agg_0_0_bias"):
        g = grads[name]
        idxs = [tuple(rng.integers(0, s) for s in g.shape) for _ in range(4)]
        # make sure at least one touched entity row is probed
        if name == "entity_emb_matrix":
            idxs[0] = (int(case.items[0]), 2)
        for idx in idxs:
            eps = 1e-4
            up, dn = dict(p64), dict(p64)
            up[name] = p64[name].copy(); up[name][idx] += eps
            dn[name] = p64[name].copy(); dn[name][idx] -= eps
            fd = (loss64(up) - loss64(dn)) / (2 * eps)
            assert abs(fd - g[idx]) <= 2e-3 * abs(fd) + 2e-6, (name, idx, fd, g[idx])


def test_adam_rule():
    params = {"w": np.array([1.0, -2.0, 0.5], np.float32)}
    opt = train_ref.AdamRef(params, lr=0.1)
    g = {"w": np.array([0.5, 0.0, -1.0], np.float32)}
    p1 = opt.step(dict(params), g)
    # first step: m_hat = g, v_hat = g^2  ->  step = lr * g / (|g| + eps')  ~ lr * sign(g)
    np.testing.assert_allclose(p1["w"], [0.9, -2.0, 0.6], atol=1e-6)
    w1 = p1["w"].copy()
    p2 = opt.step(dict(p1), {"w": np.zeros(3, np.float32)})  # zero gradient still moves (m decays, not zero)
    assert p2["w"][0] < w1[0] and p2["w"][1] == -2.0


def test_float64_route_agrees_with_the_pinned_float32_route():
    """loss_and_grads(dtype=torch.float64) is the float32 graph widened, nothing else: on a toy case the two agree to
    float32 round-off (a few hundred float32 operations per output: 1e-5 of each gradient's largest entry), the
    same parameters receive a gradient, and the float64 route does return float64."""
    args, case, params, labels = setup()
    feed = (case.adj_entity, case.adj_relation, case.users, case.items, labels, case.memories_h, case.memories_r,
            case.memories_t)
    l32, g32, p32, o32 = train_ref.loss_and_grads(args, params, *feed)
    l64, g64, p64, o64 = train_ref.loss_and_grads(args, params, *feed, dtype=torch.float64)
    assert o32.scores.dtype == torch.float32 and o64.scores.dtype == torch.float64
    assert abs(l32 - l64) <= 2e-6 * abs(l64)
    for k in p64:
        assert abs(p32[k] - p64[k]) <= 2e-6 * abs(p64[k]) + 1e-9, k
    assert set(g32) == set(g64)
    differs = False
    for k, g in g64.items():
        assert g.dtype == np.float64 and g32[k].dtype == np.float32, k
        err = np.abs(g32[k] - g).max()
        assert err <= 1e-5 * np.abs(g).max() + 1e-9, (k, err)
        differs |= bool(err > 0)
    assert differs                                  # the float64 route is not the float32 one relabelled
    np.testing.assert_allclose(o32.scores.detach().numpy(), o64.scores.detach().numpy(), rtol=0, atol=1e-5)


def test_adam_rule_in_float64_follows_the_float32_rule():
    rng = np.random.default_rng(3)
    p0 = {"w": rng.standard_normal(50).astype(np.float32)}
    a, b = train_ref.AdamRef(p0, lr=0.01), train_ref.AdamRef(p0, lr=0.01, dtype=np.float64)
    pa, pb = {"w": p0["w"].copy()}, {"w": p0["w"].astype(np.float64)}
    for _ in range(3):
        g = rng.standard_normal(50).astype(np.float32)
        pa, pb = a.step(pa, {"w": g}), b.step(pb, {"w": g})
    assert pa["w"].dtype == np.float32 and pb["w"].dtype == np.float64 and b.m["w"].dtype == np.float64
    np.testing.assert_allclose(pa["w"], pb["w"], rtol=0, atol=1e-6)
