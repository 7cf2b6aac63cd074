"""CPU: tests/l2_ref.py -- the plain float64 statement of mvin_gather_attn_l2_fwd's contract -- pinned against the per-level references
of tests/fwd_ref.py composed level by level, against fold_ref.fold_reference, against the fp32 mirror of the reference graph with
User_orient off (ablation no_uo: the W1 = W2 = None formulas), and the case builders of tests/l2_cases.py held to the conditions that
keep a case of tests/test_gpu_l2_f64.py from passing vacuously (the GPU module asserts the same conditions, through the same function,
on the float64 reference of every case it runs: the references of its large fan-outs are device work)."""
import numpy as np
import pytest
import torch

import fwd_ref
import l2_cases as lc
from bwd_ref import softmax
from fold_ref import clamp_ids, fold_reference
from l2_ref import l2_reference

CPU = "cpu"
SHAPES = [(D, K) for D in (4, 16) for K in (2, 3, 4)]


def _random_world(D, K, seed, n_entity=23, nR=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * 0.5         # noqa: E731
    adj_e = torch.randint(0, n_entity, (n_entity, K), generator=g, dtype=torch.int32)
    adj_r = torch.randint(0, nR, (n_entity, K), generator=g, dtype=torch.int32)
    return dict(E=r(n_entity, D), adj_e=adj_e, adj_r=adj_r, t0=r(nR) * 2, t1=r(nR) * 2, W1=r(D, D), W2=r(D, D), b1=r(D), b2=r(D), A0=r(D, D),
                a0=r(D), n_entity=n_entity, nR=nR, g=g)


def _options(i):
    """(t0, t1, projection, b1, b2, a0) present, rotated."""
    return dict(t0=i % 4 in (0, 1), t1=i % 4 in (0, 2), proj=i % 3 != 2, b1=i % 2 == 0, b2=i % 5 != 1, a0=i % 7 != 3)


def _call(w, parents, q, B, ppp, K, o, **kw):
    pick = lambda name, on: w[name] if on else None           # noqa: E731
    return l2_reference(w["E"], w["adj_e"], w["adj_r"], parents, pick("t0", o["t0"]), pick("t1", o["t1"]), pick("W1", o["proj"]),
                        pick("W2", o["proj"]), pick("b1", o["b1"]), pick("b2", o["b2"]), q, w["A0"], pick("a0", o["a0"]), B, ppp, K, **kw)


@pytest.mark.parametrize("ppp", [1, 3, "K"])
@pytest.mark.parametrize("D,K", SHAPES)
def test_against_the_per_level_references_composed(D, K, ppp):
    """expand_ids, then fwd_ref.agg at level L - 1 (gather form: Wc = W2, c_child = c2, N = K x parents_per_pair children per pair), then
    the two weighted sums at level L - 2 -- every option combination, parents out of range among them."""
    ppp = K if ppp == "K" else ppp
    for i in range(12):
        w = _random_world(D, K, 100 * D + 10 * K + i)
        o = _options(i)
        B = (1, 2, 5)[i % 3]
        P = B * ppp
        parents = torch.randint(0, w["n_entity"], (P,), generator=w["g"])
        parents[0] = w["n_entity"] + 7                        # clamps to the last row
        q = torch.randn(B, D, generator=w["g"])
        n0, n1, pp, pc = _call(w, parents, q, B, ppp, K, o)
        f = lambda name: w[name].double().numpy()             # noqa: E731
        x = clamp_ids(parents, w["n_entity"]).numpy()
        ents, rels = fwd_ref.expand_ids(f("adj_e"), f("adj_r"), x, K, 2, w["n_entity"])
        x1 = ents[1].reshape(-1)                              # [P * K]
        t0, t1 = (f("t0") if o["t0"] else None), (f("t1") if o["t1"] else None)
        if o["proj"]:
            qd = q.double().numpy()
            c1 = qd @ f("W1") + (f("b1") if o["b1"] else 0)
            c2 = qd @ f("W2") + (f("b2") if o["b2"] else 0)
            self1 = f("E")[x1] @ f("W1") + np.repeat(c1, K * ppp, axis=0)
            level = fwd_ref.agg(self1, f("A0"), f("a0") if o["a0"] else None, K, table=f("E"), adj_entity=f("adj_e"), adj_relation=f("adj_r"),
                                node_ids=x1, rel_score=t0, Wc=f("W2"), c_child=c2, N=K * ppp)
        else:
            self1 = f("E")[x1]
            level = fwd_ref.agg(self1, f("A0"), f("a0") if o["a0"] else None, K, table=f("E"), adj_entity=f("adj_e"), adj_relation=f("adj_r"),
                                node_ids=x1, rel_score=t0, N=K * ppp)
        p0 = softmax(t0[rels[0]]) if o["t0"] else np.ones((P, K))
        p1 = softmax(t1[rels[0]]) if o["t1"] else np.ones((P, K))
        want0 = np.einsum("pk,pkd->pd", p0, self1.reshape(P, K, D)) / K
        want1 = np.einsum("pk,pkd->pd", p1, level["out"].reshape(P, K, D)) / K
        np.testing.assert_allclose(n0.numpy(), want0, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(n1.numpy(), want1, rtol=1e-12, atol=1e-13)
        if o["t0"]:
            np.testing.assert_allclose(pp.numpy(), p0, rtol=1e-13, atol=0)
            np.testing.assert_allclose(pc.numpy(), level["probs"], rtol=1e-13, atol=0)
            assert float((pp.sum(1) - 1).abs().max()) < 1e-14 and float((pc.sum(1) - 1).abs().max()) < 1e-14
        else:
            assert pp is None and pc is None


@pytest.mark.parametrize("D,K", SHAPES)
def test_against_the_folded_reference_at_one_parent_per_pair(D, K):
    for i in range(8):
        w = _random_world(D, K, 7000 + 100 * D + 10 * K + i)
        g = w["g"]
        B = 6
        items = torch.randint(-3, w["n_entity"] + 3, (B,), generator=g)
        q, uo = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
        W0, A1, Wmix = torch.randn(D, D, generator=g), torch.randn(D, D, generator=g), torch.randn(3 * D, D, generator=g)
        o = dict(_options(i), proj=True)
        pick = lambda name, on: w[name] if on else None       # noqa: E731
        want = fold_reference(w["E"], w["adj_e"], w["adj_r"], items, pick("t0", o["t0"]), pick("t1", o["t1"]), q, uo, W0, None, w["W1"],
                              pick("b1", o["b1"]), w["W2"], pick("b2", o["b2"]), w["A0"], pick("a0", o["a0"]), A1, None, Wmix, None, K)[:2]
        got = _call(w, items, q, B, 1, K, o)[:2]
        for a, b in zip(got, want):
            torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("D,K", SHAPES)
def test_no_logits_are_weights_of_one_not_a_softmax_of_zeros(D, K):
    """include/mvin_hip.h: an absent table means p = 1 (sum_k p = K), zero logits mean p = 1 / K.  So nagg0 without t0 is K x nagg0 with
    t0 = 0, nagg1 without t1 is K x nagg1 with t1 = 0 (the same t0), and without the projection Z - self1 = S / K is K times larger too."""
    w = _random_world(D, K, 31 * D + K)
    B, ppp = 4, 3
    parents = torch.randint(0, w["n_entity"], (B * ppp,), generator=w["g"])
    q = torch.randn(B, D, generator=w["g"])
    zero = dict(w, t0=torch.zeros(w["nR"]), t1=torch.zeros(w["nR"]))
    on = dict(t0=True, t1=True, proj=True, b1=True, b2=True, a0=True)
    none0 = _call(w, parents, q, B, ppp, K, dict(on, t0=False))
    zero0 = _call(zero, parents, q, B, ppp, K, on)
    torch.testing.assert_close(none0[0], K * zero0[0], rtol=1e-13, atol=1e-14)
    assert none0[2] is None and torch.equal(zero0[2], torch.full((B * ppp, K), 1.0 / K, dtype=torch.float64))
    none1 = _call(zero, parents, q, B, ppp, K, dict(on, t1=False))
    torch.testing.assert_close(none1[1], K * zero0[1], rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(none1[0], zero0[0], rtol=0, atol=0)
    # without the projection, on a non-negative table with A0 = 1 and no a0 the ReLU is the identity and out1 = Z = self1 + S / K:
    # the children's share of Z grows by exactly K from zero logits (p = 1 / K) to no logits (p = 1)
    pos = dict(w, E=w["E"].abs(), A0=torch.eye(D))
    off = dict(on, proj=False, a0=False)
    a = _call(pos, parents, q, B, ppp, K, dict(off, t0=False), parts=True)[4]
    b = _call(dict(pos, t0=zero["t0"]), parents, q, B, ppp, K, off, parts=True)[4]
    assert torch.equal(a["self1"], b["self1"]) and float((a["out1"] - a["self1"]).min()) > 0
    torch.testing.assert_close(a["out1"] - a["self1"], K * (b["out1"] - b["self1"]), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D,K", SHAPES)
def test_chunks_of_one_parent_and_of_all_give_equal_bits(D, K, dtype):
    w = _random_world(D, K, 17 * D + K)
    B, ppp = 5, 3
    parents = torch.randint(0, w["n_entity"], (B * ppp,), generator=w["g"])
    q = torch.randn(B, D, generator=w["g"])
    for i in range(4):
        one = _call(w, parents, q, B, ppp, K, _options(i), chunk=1, dtype=dtype)
        every = _call(w, parents, q, B, ppp, K, _options(i), chunk=B * ppp, dtype=dtype)
        for a, b in zip(one, every):
            assert (a is None and b is None) or (a.dtype == dtype and torch.equal(a, b))


def test_ids_are_low_words_clamped_and_queries_go_by_pair():
    D, K = 4, 2
    w = _random_world(D, K, 5)
    n = w["n_entity"]
    ids = torch.tensor([3, n, n + 5, -1, -2 ** 31, 2 ** 32 + 4, 2 ** 40 + 1, -2 ** 32, 7])
    assert clamp_ids(ids, n).tolist() == [3, n - 1, n - 1, n - 1, n - 1, 4, 1, 0, 7]
    B, ppp = 3, 3
    q = torch.randn(B, D, generator=w["g"])
    on = dict(t0=True, t1=True, proj=True, b1=True, b2=True, a0=True)
    got = _call(w, ids, q, B, ppp, K, on)
    want = _call(w, clamp_ids(ids, n), q, B, ppp, K, on)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # parent i reads query row i // parents_per_pair: the same parents one per pair with the rows repeated
    rep = _call(w, ids, q.repeat_interleave(ppp, 0), B * ppp, 1, K, on)
    assert all(torch.equal(a, b) for a, b in zip(got, rep))


def test_a_bf16_table_widens_exactly_and_magnitude_bounds_the_value():
    D, K = 16, 4
    w = _random_world(D, K, 9)
    B = 7
    parents = torch.randint(0, w["n_entity"], (B,), generator=w["g"])
    q = torch.randn(B, D, generator=w["g"])
    on = dict(t0=True, t1=True, proj=True, b1=True, b2=True, a0=True)
    half = dict(w, E=w["E"].to(torch.bfloat16))
    wide = dict(w, E=w["E"].to(torch.bfloat16).float())
    assert all(torch.equal(a, b) for a, b in zip(_call(half, parents, q, B, 1, K, on), _call(wide, parents, q, B, 1, K, on)))
    val, mag = _call(w, parents, q, B, 1, K, on), _call(w, parents, q, B, 1, K, on, magnitude=True)
    assert bool((val[0].abs() <= mag[0]).all()) and bool((val[1].abs() <= mag[1] * (1 + 1e-15)).all())
    assert torch.equal(val[2], mag[2]) and torch.equal(val[3], mag[3])


def test_user_orient_off_is_the_raw_embedding_form():
    """W1 = W2 = None against the fp32 mirror of the reference graph evaluated in float64 with ablation no_uo (h_hop = 2, n_mix_hop = 1):
    self1 = table[x1], Z = self1 + S / K.  The mirror's stages give relu((E[x] + nagg0) A0 + a0), out1 and relu((stage + nagg1) A1 + a1)."""
    from mvin_amd import synth
    from mvin_amd.config import make_args
    from mvin_amd.params import init_params
    from oracle import mirror_fp32
    D, K, B = 8, 4, 9
    args = make_args(dim=D, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=4, batch_size=B, ablation="no_uo")
    assert not args.User_orient and args.User_orient_rela
    case = synth.small_case(args, n_user=5, n_entity=40, n_relation=6, seed=3, zero_rows=1, repeats=True)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=4, random_agg_bias=True)
    m = mirror_fp32.forward(args, params, case.adj_entity, case.adj_relation, case.users, case.items, case.memories_h, case.memories_r,
                            case.memories_t, trace=True, dtype=torch.float64)
    p = mirror_fp32.as_torch_params(params, torch.float64)
    E, rel = p["entity_emb_matrix"], p["relation_emb_matrix"]
    t0 = rel @ p["agg_0_0_urh_weights"].reshape(-1)[D:2 * D]
    t1 = rel @ p["agg_1_0_urh_weights"].reshape(-1)[D:2 * D]
    A0, a0, A1, a1 = p["agg_0_0_weights"], p["agg_0_0_bias"], p["agg_1_0_weights"], p["agg_1_0_bias"]
    items = torch.as_tensor(case.items).long()
    adj_e, adj_r = torch.as_tensor(case.adj_entity), torch.as_tensor(case.adj_relation)
    n0, n1, pp, pc, extra = l2_reference(E, adj_e, adj_r, items, t0, t1, None, None, None, None, None, A0, a0, B, 1, K, parts=True)
    stages = m.trace["stages"][0]
    torch.testing.assert_close(extra["out1"], stages[1][1], rtol=1e-12, atol=1e-13)
    stage0 = torch.relu((E[items] + n0) @ A0 + a0)
    torch.testing.assert_close(stage0, stages[1][0].reshape(B, D), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(torch.relu((stage0 + n1) @ A1 + a1), stages[2][0].reshape(B, D), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(pp, m.importance_list[0].reshape(B, K), rtol=1e-12, atol=0)
    torch.testing.assert_close(pc, m.importance_list[1].reshape(B * K, K), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------- the case builders of the GPU module
@pytest.mark.parametrize("K", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("kind", ["counts", "uniform"])
def test_real_valued_cases_meet_their_conditions(kind, K):
    """Every regime x parents per pair x (biases, projection, bf16) of the GPU module at D = 16 (and D = 32 at K = 16; at K = 64 one
    option set per regime: a reference over 256 parents is 17 M terms there, and K >= 128 is device work): ReLU share, the
    sharp rows, the unit weights, every distinct-children count among parents and children, probabilities that sum to 1."""
    for D in ((16, 32) if K == 16 else (16,)):
        w = lc.world(D, K, lc.N_ENTITY, lc.N_REL, kind, False, CPU)
        assert (w.adj_e >= 0).all() and (w.adj_e < w.n_entity).all() and (w.adj_r >= 0).all() and (w.adj_r < w.nR).all()
        assert (w.adj_e[0] == 0).all() and (w.adj_r[0] == 0).all() and w.cnt[0] == 1
        assert (w.cnt[1:] == K).all() if kind == "uniform" else (w.cnt[1:] == np.arange(1, w.n_entity) % K + 1).all()
        for regime in lc.REAL_REGIMES:
            options = ((1, True, True, False), (3, False, True, True), (K, True, False, False))
            for ppp, bias, proj, bf16 in options[:1 if K == 64 else 3]:
                c = lc.make_case(w, regime, 5, ppp, bias=bias, proj=proj, bf16=bf16)
                assert int(c.parents_ext[0]) == 0 and c.Px >= 256
                r = lc.references(c)
                assert not r["problems"], f"D={D} K={K} {kind} {regime} ppp={ppp}: {r['problems']}"
                assert all(y is None or y > 0 for y in r["yard"])
        t0, t1 = lc.logits(w, "offset")
        assert float(t0.min()) > 9990 and float((t0 - 1.0e4).abs().max()) < 4


@pytest.mark.parametrize("nR", [1, 4000, 4096])
def test_relation_counts_at_the_ends(nR):
    w = lc.world(32, 16, lc.N_ENTITY if nR == 1 else 2600, nR, "counts", False, CPU)
    for regime in ("unit", "sharp130", "none"):
        c = lc.make_case(w, regime, 5)
        assert not lc.references(c)["problems"]
    if nR == 1:
        assert bool((lc.references(lc.make_case(w, "unit", 5))["r64"][2] == 1.0 / 16).all())


@pytest.mark.parametrize("K", [4, 8, 16])
@pytest.mark.parametrize("regime", lc.EXACT_REGIMES)
def test_exact_cases_meet_their_preconditions(regime, K):
    for D in (16, 32):
        w = lc.world(D, K, lc.N_ENTITY, lc.N_REL, "planted" if regime == "planted" else "counts", True, CPU)
        for ppp, bias, proj, bf16 in ((1, True, True, False), (3, False, True, True), (K, True, False, False)):
            c = lc.make_case(w, regime, 5, ppp, bias=bias, proj=proj, bf16=bf16)
            r = lc.references(c)
            assert not r["problems"], r["problems"]
            assert not lc.exact_precondition(c, r["r64"])
            if regime == "planted":
                assert set(np.unique(r["r64"][2].numpy())) <= {0.0, 0.25, 0.5, 1.0, 1.0 / K}
                # fp32 evaluates the planted weights exactly too
                assert torch.equal(r["r32"][2].double(), r["r64"][2]) and torch.equal(r["r32"][0].double(), r["r64"][0])


def test_the_exact_levels_hold_for_the_large_fan_outs():
    """The worst-case magnitude of out1 under the value ranges of each level, against 2^24 / (4 K^2)."""
    for K in (4, 8, 16, 32, 64, 128, 256):
        tv, wv, nnz = lc.EXACT_LEVELS[lc.exact_level(K)]
        self1 = 2 * tv * nnz * wv + tv
        Z = self1 + tv * nnz * wv + (tv * nnz * wv + tv)
        out1 = Z * nnz * wv + tv
        assert out1 * 4 * K * K < 2 ** 24, (K, out1)
