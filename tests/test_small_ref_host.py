"""tests/small_ref.py -- the float64 statement of mvin_score_small_fwd's contract -- against the float64 oracle of the reference graph
(oracle/equations_fp64.py through parity.run_oracles) on small model cases at the scale of a trained model (the TRAINED multipliers of
tests/test_gpu_small_sharp.py), tree depths 1 and 2, the ablations that reach the kernel as pointer patterns; its id rules; its fp32
evaluation; its magnitude form; and the conditions of tests/small_cases.py on the reference alone.  CPU only."""
import numpy as np
import pytest
import torch

import small_cases as sc
import small_ref as sr
from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from parity import run_oracles

TRAINED = {"entity_emb_matrix": 25.0, "relation_emb_KGE_matrix": 6.0, "relation_emb_matrix": 6.0, "user_emb_matrix": 2.0, "urh_weights": 6.0}


def trained(params):
    out = dict(params)
    for k, v in params.items():
        for tag, f in TRAINED.items():
            if k == tag or (tag == "urh_weights" and k.endswith(tag)):
                out[k] = (np.asarray(v) * np.float32(f)).astype(np.float32)
    return out


def tensors_of(args, params, depth):
    """The kernel's arguments from a model's parameter dict (MVIN._score_args_static / _score_small_native)."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))        # noqa: E731
    D = args.dim
    p = params
    uo = args.User_orient
    rel = p["relation_emb_matrix"]
    # t[r] = relation_emb[r] . urh_weights[D:2D] (the k-dependent term of aggregators.py:130-133), in float64: the table is an INPUT of the kernel
    logit = lambda i: t(rel.astype(np.float64) @ p[f"agg_{i}_0_urh_weights"][D:2 * D, 0].astype(np.float64)) if args.User_orient_rela else None      # noqa: E731
    W = [t(p[f"transfer_matrix_{e}"]) if (uo and e <= depth) else None for e in range(3)]
    b = [t(p[f"transfer_bias_{e}"]) if (uo and e <= depth) else None for e in range(3)]
    two = depth == 2
    return dict(E=t(p["entity_emb_matrix"]), R=t(p["relation_emb_KGE_matrix"]), w_h=t(p["h_emb_item_mlp_matrix"][:D, 0]) if args.PS_O_ft else None,
                Wu=t(p["user_mlp_matrix"]), bu=t(p["user_mlp_bias"]), t0=logit(0), t1=logit(1) if two else None,
                W0=W[0], b0=b[0], W1=W[1], b1=b[1], W2=W[2], b2=b[2], A0=t(p["agg_0_0_weights"]), a0=t(p["agg_0_0_bias"]),
                A1=t(p["agg_1_0_weights"]) if two else None, a1=t(p["agg_1_0_bias"]) if two else None,
                Wmix=t(p["enti_transfer_matrix_0"]), bmix=t(p["enti_transfer_bias_0"]))


def call(k, case, P, K, nR, depth, dtype=torch.float64, items=None, mem=None, users=None, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    mem = mem if mem is not None else tuple([t(m) for m in lst] for lst in (case.memories_h, case.memories_r, case.memories_t))
    return sr.small_reference(k["E"], t(case.adj_entity), t(case.adj_relation), k["R"], k["w_h"], k["Wu"], k["bu"], k["t0"], k["t1"], k["W0"], k["b0"],
                              k["W1"], k["b1"], k["W2"], k["b2"], k["A0"], k["a0"], k["A1"], k["a1"], k["Wmix"], k["bmix"],
                              t(case.items) if items is None else items, mem, users, P, K, nR, depth=depth, dtype=dtype, **kw)


def model_case(D, K, P, Nm, nR, B, depth, ablation, seed):
    args = make_args(dim=D, neighbor_sample_size=K, h_hop=depth, n_mix_hop=1, p_hop=P, n_memory=Nm, batch_size=B, ablation=ablation)
    case = synth.small_case(args, n_user=7, n_entity=90, n_relation=nR, seed=seed, zero_rows=3, repeats=True)
    uts = synth.ripple_sets(7, 90, nR, P, Nm, seed=seed + 1)
    case.memories_h, case.memories_r, case.memories_t = synth.memories_for(uts, case.users)
    params = trained(init_params(args, case.n_user, case.n_entity, case.n_relation, seed=seed + 2, random_agg_bias=True))
    return args, case, params, uts


@pytest.mark.parametrize("ablation", ["all", "no_uor", "no_uo", "no_ps_o_ft"])
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("shape", [(16, 4, 2, 5, 5), (8, 3, 1, 17, 3), (32, 5, 3, 4, 4)], ids=lambda s: "D%dK%dP%dNm%dnR%d" % s)
def test_equals_the_float64_oracle(shape, depth, ablation):
    D, K, P, Nm, nR = shape
    B = 9
    args, case, params, uts = model_case(D, K, P, Nm, nR, B, depth, ablation, seed=D + K + depth)
    _, e = run_oracles(args, case, params)
    k = tensors_of(args, params, depth)
    assert (k["t0"] is None) == (ablation == "no_uor") and (k["W0"] is None) == (ablation == "no_uo") and (k["w_h"] is None) == (ablation == "no_ps_o_ft")
    assert float(np.abs(e.scores).max()) >= 1, "not the scale of a trained model"
    for feed in ("lists", "users"):
        r = call(k, case, P, K, nR, depth) if feed == "lists" else call(k, case, P, K, nR, depth, mem=torch.from_numpy(uts), users=torch.from_numpy(case.users))
        for name, ref in (("user_o", e.user_o), ("item_emb", e.item_embeddings), ("scores", e.scores), ("sigmoid", e.scores_normalized)):
            got, ref = getattr(r, name), torch.from_numpy(np.asarray(ref, dtype=np.float64))
            assert got.dtype == torch.float64 and got.shape == ref.shape
            err = float(((got - ref).abs() / (1 + ref.abs())).max())
            assert err <= 1e-11, f"{feed} {name}: {err:.3e}"


def test_float32_evaluation_is_float32_and_close():
    args, case, params, _ = model_case(16, 4, 2, 5, 5, 9, 2, "all", seed=3)
    k = tensors_of(args, params, 2)
    hi, lo = call(k, case, 2, 4, 5, 2), call(k, case, 2, 4, 5, 2, dtype=torch.float32)
    for name in ("user_o", "item_emb", "scores", "sigmoid"):
        a, b = getattr(hi, name), getattr(lo, name)
        assert b.dtype == torch.float32
        err = float(((b.double() - a).abs() / (1 + a.abs())).max())
        assert 0 < err < 1e-4, name


def test_id_rules():
    """Items whole as unsigned 64-bit; memory and relation ids as unsigned words; users signed."""
    n = 90
    assert sr.clamp_item_ids(torch.tensor([3, -1, n, (1 << 32) + 4, -(1 << 40), n - 1]), n).tolist() == [3, n - 1, n - 1, n - 1, n - 1, n - 1]
    assert sr.clamp_words(torch.tensor([3, -1, n + 5, -2 ** 31], dtype=torch.int32), n).tolist() == [3, n - 1, n - 1, n - 1]
    assert sr.clamp_users(torch.tensor([-5, 0, 6, 7, 1 << 40]), 7).tolist() == [0, 0, 6, 6, 6]
    args, case, params, uts = model_case(16, 4, 2, 5, 5, 9, 2, "all", seed=4)
    k = tensors_of(args, params, 2)
    items = torch.from_numpy(case.items).clone()
    users = torch.from_numpy(case.users).clone()
    bad_uts = torch.from_numpy(uts).clone()
    good_items, good_users, good_uts = items.clone(), users.clone(), bad_uts.clone()
    items[1], good_items[1] = -3, n - 1
    items[2], good_items[2] = (1 << 32) + 1, n - 1
    users[3], good_users[3] = -2, 0
    users[4], good_users[4] = 7 + 11, 6
    bad_uts[:, 0, 0, 1], good_uts[:, 0, 0, 1] = -1, n - 1
    bad_uts[:, 1, 2, 0], good_uts[:, 1, 2, 0] = n + 7, n - 1
    bad_uts[:, 0, 1, 2], good_uts[:, 0, 1, 2] = 5 + 3, 4
    a = call(k, case, 2, 4, 5, 2, items=items, mem=bad_uts, users=users)
    b = call(k, case, 2, 4, 5, 2, items=good_items, mem=good_uts, users=good_users)
    c = call(k, case, 2, 4, 5, 2, mem=torch.from_numpy(uts), users=torch.from_numpy(case.users))
    assert torch.equal(a.scores, b.scores) and torch.equal(a.user_o, b.user_o) and not torch.equal(a.scores, c.scores)


def test_an_adjacency_without_relations_reads_relation_zero():
    args, case, params, _ = model_case(16, 4, 2, 5, 5, 9, 2, "all", seed=5)
    k = tensors_of(args, params, 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    mem = tuple([t(m) for m in lst] for lst in (case.memories_h, case.memories_r, case.memories_t))
    args_ = (k["E"], t(case.adj_entity))
    rest = (k["R"], k["w_h"], k["Wu"], k["bu"], k["t0"], k["t1"], k["W0"], k["b0"], k["W1"], k["b1"], k["W2"], k["b2"], k["A0"], k["a0"], k["A1"],
            k["a1"], k["Wmix"], k["bmix"], t(case.items), mem, None, 2, 4, 5)
    none = sr.small_reference(*args_, None, *rest)
    zero = sr.small_reference(*args_, torch.zeros_like(t(case.adj_relation)), *rest)
    real = sr.small_reference(*args_, t(case.adj_relation), *rest)
    assert torch.equal(none.scores, zero.scores) and not torch.equal(none.scores, real.scores)


def test_magnitude_bounds_every_output():
    args, case, params, _ = model_case(16, 4, 2, 5, 5, 9, 2, "all", seed=6)
    for depth in (1, 2):
        args, case, params, _ = model_case(16, 4, 2, 5, 5, 9, depth, "all", seed=6)
        k = tensors_of(args, params, depth)
        r, m = call(k, case, 2, 4, 5, depth), call(k, case, 2, 4, 5, depth, magnitude=True)
        for name in ("user_o", "item_emb", "scores"):
            assert bool((getattr(r, name).abs() <= getattr(m, name) * (1 + 1e-12)).all()), name


@pytest.mark.parametrize("user_regime", sc.kr.REGIMES)
def test_real_cases_meet_their_conditions_on_the_reference(user_regime):
    """One small world per user-side regime, every tree-side regime, both depths: the conditions of small_cases.conditions on the float64
    reference (what tests/test_gpu_small_f64.py asserts for every case it runs)."""
    w = sc.world(16, 4, 17, 2, 5, user_regime, "counts", True, "cpu")
    for i, regime in enumerate(sc.lc.REAL_REGIMES):
        c = sc.make_case(w, regime, 9, depth=2 - i % 2)
        refs = sc.references(c)
        assert not refs["problems"], f"{user_regime} {regime}: {refs['problems']}"
        assert all(v > 0 for v in refs["yard"].values())


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("K", [4, 8])
def test_exact_cases_meet_their_precondition(K, depth):
    for regime in sc.lc.EXACT_REGIMES:
        w = sc.exact_world(16, K, 16, 2, 5, regime, True, "cpu")
        c = sc.make_case(w, regime, 37, depth=depth)
        refs = sc.references(c)
        assert not refs["problems"], refs["problems"]
        pre = sc.exact_precondition(c, refs["r64"], sc.OUTPUTS[:3])
        assert not pre, pre
