"""-m gpu: the single-launch pass (mvin_score_small_fwd: a row's memories split into SP parts, merged by exp(m_i - M)) and the model's
dispatch (flash key addressing, the kernel over records, the single launch) at the scale of a TRAINED model.

Every whole-model test uses init_params as it comes: Xavier at initialisation, entity rows of +-0.06, ripple logits of order 3e-3, scores of
order 1e-2 -- every softmax a plain mean, every merge weight 1.  Here the tables are multiplied by TRAINED (entity rows x 25, R_KGE x 6,
relation embeddings x 6, user embeddings x 2, every urh_weights x 6; chosen on the CPU from oracle/equations_fp64.py) and each case asserts, on
the float64 oracle's own output, that the regime is a trained model's: at least half of the ripple rows have a top probability of 0.5 or
more, the relation-attention logits of at least half of the rows spread by more than 5, and max |score| >= 5.

Rule: per output (user_o, item_embeddings, scores, sigmoid) err_hip = max |HIP - float64| <= 4 err_mirror + 1e-6, err_mirror = max |fp32 mirror
of the reference graph on the same parameters - float64| (parity.check_case's rule).  The mirror's own rtol 1e-5 / atol 1e-6 is not asserted:
at scores of 5 and more it is below one ulp.  Scores are bit-equal between the per-pair and the users feed.

MEASURED on an MI355X, worst err_hip / (4 err_mirror + 1e-6) over the group sizes and both feeds (err_hip | err_mirror | ratio):
    single launch, D64 K32 Nm64    user_o 2.1e-6 | 4.6e-6 | 0.11   item 2.5e-6 | 4.9e-6 | 0.12   scores 1.8e-5 | 2.9e-5 | 0.15   sigmoid 2.1e-6 | 2.0e-6 | 0.23
    single launch, D32 K16 Nm64    user_o 2.5e-6 | 2.5e-6 | 0.23   item 2.1e-6 | 2.2e-6 | 0.21   scores 1.0e-5 | 1.4e-5 | 0.18   sigmoid 1.5e-6 | 6.0e-7 | 0.45
    single launch, D16 K8 Nm64     user_o 1.0e-6 | 2.0e-6 | 0.12   item 1.3e-6 | 2.0e-6 | 0.15   scores 7.8e-6 | 3.7e-6 | 0.49   sigmoid 1.5e-6 | 5.6e-7 | 0.46
    single launch, D64 K8 P3 Nm8   user_o 4.9e-6 | 4.1e-6 | 0.28   item 3.7e-6 | 4.7e-6 | 0.18   scores 4.2e-5 | 3.6e-5 | 0.28   sigmoid 3.0e-6 | 3.6e-6 | 0.19
    single launch, D64 K32 Nm40    user_o 1.9e-6 | 6.3e-6 | 0.07   item 2.2e-6 | 4.2e-6 | 0.12   scores 7.4e-6 | 1.1e-5 | 0.17   sigmoid 1.2e-6 | 6.2e-7 | 0.35
    forward_users, 700 pairs (|score| up to 82): single launch 0.17, flash key addressing 0.37, kernel over records 0.26 (worst output each)
Run with -s for the figures of a run (lines starting with MEASURED).  6 cases, 24 s, most of it the CPU oracles.

That the module bites: on a scratch copy with the merge weight of the single launch's parts (w = lean_exp(m_i - M)) replaced by 1, the shapes
whose rows are split (D 64, K 32, Nm 64 and Nm 40; the 700-pair batch) fail with user_o 1.9 .. 4.6 and scores 10 .. 70 off; the same copy moves
test_gpu_small.py's scores, at initialisation scale, by 1e-4.
"""
import numpy as np
import pytest
import torch

import keyaddr_ref as kr
from mvin_amd import ops, synth
from mvin_amd.config import make_args
from mvin_amd.model import MVIN
from mvin_amd.params import init_params

from parity import run_oracles

pytestmark = pytest.mark.gpu

TRAINED = {"entity_emb_matrix": 25.0, "relation_emb_KGE_matrix": 6.0, "relation_emb_matrix": 6.0, "user_emb_matrix": 2.0, "urh_weights": 6.0}
# (D, K, P, Nm, nR, B)
SHAPES = [(64, 32, 2, 64, 9, 37), (32, 16, 2, 64, 12, 37), (16, 8, 2, 64, 9, 37), (64, 8, 3, 8, 5, 37), (64, 32, 2, 40, 9, 9)]
OUTPUTS = ("user_o", "item_embeddings", "scores", "scores_normalized")


def trained(params):
    out = dict(params)
    for k, v in params.items():
        for tag, f in TRAINED.items():
            if k == tag or (tag == "urh_weights" and k.endswith(tag)):
                out[k] = (np.asarray(v) * np.float32(f)).astype(np.float32)
    return out


def assert_trained_regime(args, case, params, e):
    """The three conditions, in float64: from the oracle's output, the ripple rows' probabilities from tests/keyaddr_ref.py on the same tables."""
    t = lambda x: torch.from_numpy(np.asarray(x))             # noqa: E731
    mem = tuple([t(m) for m in lst] for lst in (case.memories_h, case.memories_r, case.memories_t))
    r = kr.keyaddr_reference(t(params["entity_emb_matrix"]), t(params["relation_emb_KGE_matrix"]), None, t(params["user_mlp_matrix"])[args.dim:],
                             t(params["user_mlp_bias"]), mem, t(case.users), t(case.items), args.p_hop)
    top = torch.stack(r.probs, 1).max(-1).values
    assert float((top >= 0.5).double().mean()) >= 0.5, "ripple rows: fewer than half have a top probability of 0.5"
    spread = np.concatenate([np.log(p.max(-1) / p.min(-1)).reshape(-1) for p in e.importance_list if p is not None])
    assert float((spread > 5).mean()) >= 0.5, "relation attention: fewer than half of the rows spread by more than 5"
    assert float(np.abs(e.scores).max()) >= 5, "scores: max |score| below 5"


def check(out, m, e, what, fails, stats):
    for name in OUTPUTS:
        ref = np.asarray(getattr(e, name), dtype=np.float64)
        mir = getattr(m, name).double().numpy()
        got = getattr(out, name).double().cpu().numpy()
        err_hip, err_mir = float(np.abs(got - ref).max()), float(np.abs(mir - ref).max())
        rel = err_hip / (4 * err_mir + 1e-6)
        s = stats.setdefault(name, [0.0, 0.0, 0.0])
        if rel >= s[2]:
            s[:] = [err_hip, err_mir, rel]
        if not rel <= 1.0:
            fails.append(f"{what} {name}: HIP-vs-fp64 {err_hip:.3e} > 4 x mirror-vs-fp64 {err_mir:.3e} + 1e-6 ({rel:.2f} x)")
    return {name: 4 * float(np.abs(getattr(m, name).double().numpy() - np.asarray(getattr(e, name))).max()) + 1e-6 for name in OUTPUTS}


def report(key, stats):
    for name, s in stats.items():
        print(f"MEASURED {key} {name}: err_hip {s[0]:.3e} | err_mirror {s[1]:.3e} | {s[2]:.3f}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%dK%dP%dNm%dnR%d_B%d" % s)
def test_single_launch_at_trained_scale(shape, hip_lib):
    D, K, P, Nm, nR, B = shape
    assert ops.score_small_supported(D, K, P, Nm, nR)
    args = make_args(dim=D, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=Nm, batch_size=B)
    case = synth.small_case(args, n_user=11, n_entity=1500, n_relation=nR, seed=D + K, zero_rows=5, repeats=True)
    uts = synth.ripple_sets(11, 1500, nR, P, Nm, seed=D + K + 1)
    case.memories_h, case.memories_r, case.memories_t = synth.memories_for(uts, case.users)
    params = trained(init_params(args, case.n_user, case.n_entity, case.n_relation, seed=D + K + 2, random_agg_bias=True))
    m, e = run_oracles(args, case, params)
    assert_trained_regime(args, case, params, e)
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
    model.small_max_batch = 16384                             # this module runs with MVIN_SMALL=0 (tests/conftest.py): the launch is asked for here
    dev = model.device
    users, items = torch.from_numpy(case.users).to(dev), torch.from_numpy(case.items).to(dev)
    mem = [[torch.from_numpy(x).to(dev) for x in lst] for lst in (case.memories_h, case.memories_r, case.memories_t)]
    uts_d = torch.from_numpy(uts).to(dev)
    fails, stats = [], {}
    for G in (0, 1, 4, 16):                                   # pairs per workgroup: the parts-per-row split takes every value it can
        model.small_group = G
        out = model.forward_device(users, items, *mem)
        assert model._small_state is not None and model._small_state["args"].B == B, "the single launch was expected"
        check(out, m, e, f"per-pair feed G={G}", fails, stats)
        out_u = model.forward_users(users, items, uts_d)
        check(out_u, m, e, f"users feed G={G}", fails, stats)
        assert torch.equal(out.scores, out_u.scores)          # the same reads, the same arithmetic
    report("single-launch D%dK%dP%dNm%dnR%d" % shape[:5], stats)
    assert not fails, "\n".join(fails)


def test_forward_users_schedules_at_trained_scale(hip_lib):
    """(D 64, K 4, P 2, Nm 64, nR 9), 40 users, 700 pairs: the single launch, the multi-launch schedule with the flash form of key addressing
    and without it, each under the rule, and one against the other within the sum of their bounds."""
    D, K, P, Nm, nR, n_user, B, n_entity = 64, 4, 2, 64, 9, 40, 700, 500
    args = make_args(dim=D, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=Nm, batch_size=B)
    rng = np.random.default_rng(D + Nm + B)
    adj_e, adj_r = synth.uniform_adjacency(n_entity, nR, K, seed=3)
    uts = synth.ripple_sets(n_user, n_entity, nR, P, Nm, seed=4)
    case = synth.small_case(args, n_user=n_user, n_entity=n_entity, n_relation=nR, seed=1)
    case.adj_entity, case.adj_relation = adj_e, adj_r
    case.users, case.items = rng.integers(0, n_user, B, dtype=np.int64), rng.integers(0, n_entity, B, dtype=np.int64)
    case.memories_h, case.memories_r, case.memories_t = synth.memories_for(uts, case.users)
    params = trained(init_params(args, n_user, n_entity, nR, seed=5, random_agg_bias=True))
    m, e = run_oracles(args, case, params)
    assert_trained_regime(args, case, params, e)
    model = MVIN(args, n_user, n_entity, nR, adj_e, adj_r, params=params, device="cuda:0")
    model.group_min_pairs_per_user = 0
    dev = model.device
    u_d, i_d, uts_d = torch.from_numpy(case.users).to(dev), torch.from_numpy(case.items).to(dev), torch.from_numpy(uts).to(dev)
    fails, outs, bounds = [], {}, None
    for name, small, flash in (("single launch", 1024, None), ("flash key addressing", 0, True), ("kernel over records", 0, False)):
        model.small_max_batch, model.ka_flash = small, flash
        model._small_state = None
        out = model.forward_users(u_d, i_d, uts_d)
        torch.cuda.synchronize()
        if small:
            assert model._small_state is not None and model._small_state["args"].B == B, "the single launch was expected"
        else:
            assert model._small_state is None, "the multi-launch schedule was expected"
            assert model._ka_flash_for(uts_d, model.user_records(uts_d), B) == flash
            assert ops.user_records_supported(D, P, Nm, nR)
            if flash:
                assert any(t is not None for t in model._ka_flash_ws.values()), "the flash form of key addressing was expected"
        stats = {}
        bounds = check(out, m, e, name, fails, stats)
        report("forward_users " + name.replace(" ", "-"), stats)
        outs[name] = {k: getattr(out, k).double().cpu().numpy() for k in OUTPUTS}
    names = list(outs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for k in OUTPUTS:
                d = float(np.abs(outs[a][k] - outs[b][k]).max())
                if not d <= 2 * bounds[k]:
                    fails.append(f"{a} vs {b} {k}: {d:.3e} apart, the two bounds add to {2 * bounds[k]:.3e}")
    assert not fails, "\n".join(fails)
