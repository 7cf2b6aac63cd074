"""-m gpu: the per-call entity tables of dim 64 from their own kernel (mvin_entity_tables.hip: the product computed transposed,
weights in registers, rows straight from global memory, 16-byte stores) against the kernel they came from before,
linear_mfma_kernel behind ``ops.linear`` -- BIT FOR BIT: the new kernel keeps that kernel's contraction order (step s contracts
k = 4 s .. 4 s + 3, steps ascending into one accumulator chain, + 0 at the end) with the two factors of every product swapped.
  1. every table of mvin_project_relations, mvin_key_addressing_flash_prepare and mvin_fold_tables, in poisoned workspaces with
     a guard tail; the rest of each workspace (E . w, the parameter block) against its formulas;
  2. mvin_score_l2_fwd's one launch for all tables of a step against the Python schedule's separate calls;
  3. the shapes the new kernel does not take still come from linear_mfma_kernel."""
import numpy as np
import pytest
import torch

from mvin_amd import ops, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

pytestmark = pytest.mark.gpu

D = 64
DEV = "cuda:0"
GUARD = 1024
# the launcher's grid: workgroups of four waves on four consecutive jobs, each walking row tiles of 16 entities; at most 1024
# workgroups over all job groups (mvin_entity_tables.hip: kEtRows, kEtWgCap)
TILE_ROWS, WG_CAP = 16, 1024
# one job (nR = 1, no TW): one job group, 1024 workgroups -- every one of them walks three tiles, the first few a fourth, partly filled
N_MULTI_TILE = 3 * WG_CAP * TILE_ROWS + 5 * TILE_ROWS + 3


def rnd(rng, *shape, scale=0.3):
    return torch.from_numpy((rng.normal(size=shape) * scale).astype(np.float32)).to(DEV)


def poisoned(n):
    """A workspace of n floats in front of a guard tail, all NaN."""
    buf = torch.full((n + GUARD,), float("nan"), device=DEV)
    return buf, buf[:n]


def untouched(t):
    return bool(torch.isnan(t).all())


def assert_tables_equal(got, E, mats, what):
    """got [len(mats), nE, 64] against ops.linear([E], W, 64) per matrix."""
    for i, W in enumerate(mats):
        want = ops.linear([E], W.contiguous(), D)
        assert torch.equal(got[i], want), f"{what}[{i}]: {int((got[i] != want).sum())} of {want.numel()} elements differ"


def check_hs(hs, E, w, what):
    """E . w from entity_dot_kernel: 64 products summed in fp32 in some order -- within 64 u sum |e_k w_k| of float64 (u = 2^-24)."""
    Ed, wd = E.double(), w.double()
    bound = 64 * 2.0 ** -24 * (Ed.abs() @ wd.abs()) + 1e-30
    err = (hs.double() - Ed @ wd).abs()
    assert bool((err <= bound).all()), f"{what}: E . w off by {float((err / bound).max()):.2f} x its bound"


@pytest.mark.parametrize("n_entity", [1, 15, 16, 17, 47, 4099, N_MULTI_TILE])
def test_relation_and_mlp_tables_are_bit_equal(n_entity, hip_lib):
    rng = np.random.default_rng(1000 + n_entity)
    E = rnd(rng, n_entity, D)
    big = n_entity == N_MULTI_TILE
    assert not big or n_entity > 3 * WG_CAP * TILE_ROWS          # every workgroup walks more than one tile at the grid cap
    for nR in ((1,) if big else (1, 9)):
        R = rnd(rng, nR, D, D)
        Rt = [R[r].t() for r in range(nR)]                       # ER[r] = E . R[r]^T
        tab = n_entity * D
        n_hs = (n_entity + 3) & ~3
        for has_w in (True, False):
            w = rnd(rng, D) if has_w else None
            # ---- mvin_project_relations
            n = hip_lib.mvin_project_relations_elems(n_entity, nR, D)
            assert n == nR * tab + n_hs + nR * D * D
            buf, ws = poisoned(n)
            ops.project_relations(E, R, w, out=ws)
            torch.cuda.synchronize()
            assert_tables_equal(ws[:nR * tab].view(nR, n_entity, D), E, Rt, f"ER nE={n_entity} nR={nR}")
            if has_w:
                check_hs(ws[nR * tab:nR * tab + n_entity], E, w, f"project_relations nE={n_entity}")
            else:
                assert untouched(ws[nR * tab:nR * tab + n_entity])
            assert untouched(ws[nR * tab + n_entity:]), "the padding of E . w and the scratch behind it are not written at dim 64"
            assert untouched(buf[n:]), "mvin_project_relations wrote past mvin_project_relations_elems"
            # ---- mvin_key_addressing_flash_prepare
            for P in ((1,) if big else (1, 2)):
                n_o = P + (1 if has_w else 0)
                W = rnd(rng, n_o * D, D)
                n2 = hip_lib.mvin_key_addressing_flash_tables_elems(n_entity, nR, D, P, 1 if has_w else 0)
                assert n2 == n + n_o * tab
                buf, ws = poisoned(n2)
                ops.key_addressing_flash_prepare(E, R, w, W, P, out=ws)
                torch.cuda.synchronize()
                what = f"nE={n_entity} nR={nR} P={P} w={has_w}"
                assert_tables_equal(ws[:nR * tab].view(nR, n_entity, D), E, Rt, "flash ER " + what)
                assert_tables_equal(ws[n:].view(n_o, n_entity, D), E, [W[D * j:D * j + D] for j in range(n_o)], "flash TW " + what)
                if has_w:
                    check_hs(ws[nR * tab:nR * tab + n_entity], E, w, "flash_prepare " + what)
                else:
                    assert untouched(ws[nR * tab:nR * tab + n_entity])
                assert untouched(ws[nR * tab + n_entity:n])
                assert untouched(buf[n2:]), "mvin_key_addressing_flash_prepare wrote past mvin_key_addressing_flash_tables_elems"


def fold_inputs(rng, n_entity, K, nR, dim=D):
    adj_e = torch.from_numpy(rng.integers(0, n_entity, (n_entity, K)).astype(np.int32)).to(DEV)
    adj_r = torch.from_numpy(rng.integers(0, nR, (n_entity, K)).astype(np.int32)).to(DEV)
    enc_e, enc_r, _ = ops.encode_adjacency(adj_e, adj_r)
    p = dict(W0=rnd(rng, dim, dim), W1=rnd(rng, dim, dim), W2=rnd(rng, dim, dim), A0=rnd(rng, dim, dim), A1=rnd(rng, dim, dim),
             Wmix=rnd(rng, 3 * dim, dim), b0=rnd(rng, dim), b1=rnd(rng, dim), b2=rnd(rng, dim), a0=rnd(rng, dim), bmix=rnd(rng, dim))
    return enc_e, enc_r, p


def run_fold(E, enc_e, enc_r, t0, p, K, nR, out, aggregates):
    return ops.fold_tables(E, enc_e, enc_r, t0, p["W0"], p["b0"], p["W1"], p["b1"], p["W2"], p["b2"], p["A0"], p["a0"], p["Wmix"], p["bmix"],
                           p["A1"], K, nR, out=out, aggregates=aggregates)


def check_fold_block(blk, p, c, dim=D):
    """The parameter block of mvin_fold_tables (fold_prepare_kernel): Wstack[4] | Wv | Wq | bv | bq | bm | Wperm[6].  Every product row is a
    chain of `dim` fused multiply-adds (one more for the c-weighted sums): within (dim + 2) u sum |terms| of float64; Wperm is a
    regrouped COPY (Wperm[k][c][ntp] = W[k][16 ntp + c]) of Wq | Wv | W0.Wm0 | A1 | Wm1 | Wm2: exact."""
    DD = dim * dim
    d = {k: (v.double() if v is not None else None) for k, v in p.items()}
    u = (dim + 2) * 2.0 ** -24

    def close(got, want, mag, what):
        err = (got.double() - want).abs()
        assert bool((err <= u * mag + 1e-30).all()), f"{what}: off by {float((err / (u * mag + 1e-30)).max()):.2f} x its bound"

    A0, Wm0 = d["A0"], d["Wmix"][:dim]
    prod = lambda X, Y: (X @ Y, X.abs() @ Y.abs())              # noqa: E731
    s1, m1 = prod(d["W1"], A0)
    s2, m2 = prod(d["W2"], A0)
    s0, m0 = prod(d["W0"], A0)
    sm, mm = prod(d["W0"], Wm0)
    Wstack = blk[:4 * DD].view(4, dim, dim)
    for i, (s, m, nm) in enumerate(((s1, m1, "W1.A0"), (s2, m2, "W2.A0"), (s0, m0, "W0.A0"), (sm, mm, "W0.Wm0"))):
        close(Wstack[i], s, m, nm)
    Wv, Wq = blk[4 * DD:5 * DD].view(dim, dim), blk[5 * DD:6 * DD].view(dim, dim)
    close(Wv, s1 + c * s2, m1 + c * m2, "Wv")
    close(Wq, s0 + c * s1, m0 + c * m1, "Wq")
    bv, bq, bm = (blk[6 * DD + i * dim:6 * DD + (i + 1) * dim] for i in range(3))
    vb = lambda b, Y: (b @ Y, b.abs() @ Y.abs())                # noqa: E731
    t1, n1 = vb(d["b1"], A0)
    t2, n2 = vb(d["b2"], A0)
    t0_, n0 = vb(d["b0"], A0)
    tm, nm_ = vb(d["b0"], Wm0)
    close(bv, t1 + c * t2 + d["a0"], n1 + c * n2 + d["a0"].abs(), "bv")
    close(bq, t0_ + c * t1 + d["a0"], n0 + c * n1 + d["a0"].abs(), "bq")
    close(bm, d["bmix"] + tm, d["bmix"].abs() + nm_, "bm")
    Wperm = blk[6 * DD + 3 * dim:].view(6, dim, 16, dim // 16)
    src = (Wq, Wv, Wstack[3], p["A1"], p["Wmix"][dim:2 * dim], p["Wmix"][2 * dim:])
    for i, S in enumerate(src):
        assert torch.equal(Wperm[i], S.view(dim, dim // 16, 16).transpose(1, 2)), f"Wperm[{i}]"


@pytest.mark.parametrize("n_entity", [1, 15, 16, 17, 47, 4099])
def test_folded_tables_are_bit_equal(n_entity, hip_lib):
    rng = np.random.default_rng(2000 + n_entity)
    K, nR = 16, 9
    E = rnd(rng, n_entity, D)
    enc_e, enc_r, p = fold_inputs(rng, n_entity, K, nR)
    tab, DD = n_entity * D, D * D
    n = hip_lib.mvin_fold_tables_elems(n_entity, D)
    assert n == 6 * tab + 12 * DD + 3 * D
    for aggregates in (True, False):
        for t0 in (rnd(rng, nR), None):
            buf, ws = poisoned(n)
            run_fold(E, enc_e, enc_r, t0, p, K, nR, ws, aggregates)
            torch.cuda.synchronize()
            blk = ws[6 * tab:]
            Wstack = blk[:4 * DD].view(4, D, D).clone()          # read back: the matrices the tables were built from
            assert_tables_equal(ws[:4 * tab].view(4, n_entity, D), E, list(Wstack), f"folded tables nE={n_entity} agg={aggregates}")
            check_fold_block(blk, p, (1.0 / K) if t0 is not None else 1.0)
            if aggregates:
                assert bool(torch.isfinite(ws[4 * tab:6 * tab]).all()), "H0 | G"
            else:
                assert untouched(ws[4 * tab:6 * tab]), "the gather form writes no aggregates"
            assert untouched(buf[n:]), "mvin_fold_tables wrote past mvin_fold_tables_elems"


def test_one_launch_for_all_tables_equals_the_separate_calls(hip_lib):
    """MVIN.forward_users in the flash form + the folded tail: the native call (mvin_score_l2_fwd: parameter block, then ER | TW | TA1 | TA2 |
    T0A | M0 in ONE launch, ahead of key addressing) against the Python schedule (_key_addressing_grouped + agg_fun: the flash tables,
    then key addressing, then mvin_fold_tables)."""
    from mvin_amd.model import MVIN
    B, n_user, n_entity, nR = 1500, 64, 3001, 9
    args = make_args(dim=D, neighbor_sample_size=32, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=64, batch_size=B)
    rng = np.random.default_rng(5)
    adj_e, adj_r = synth.uniform_adjacency(n_entity, nR, 32, seed=3)
    uts = synth.ripple_sets(n_user, n_entity, nR, 2, 64, seed=4)
    users = rng.integers(0, n_user, B, dtype=np.int64)
    items = rng.integers(0, n_entity, B, dtype=np.int64)
    params = init_params(args, n_user, n_entity, nR, seed=6, random_agg_bias=True)
    outs = []
    for native in (True, False):
        model = MVIN(args, n_user, n_entity, nR, adj_e, adj_r, params=params, device=DEV)
        model.group_min_pairs_per_user, model.small_max_batch, model.dedup = 0, 0, True
        model.ka_flash = model.prj = True
        if not native:
            model.native_l2_max_batch = 0
            model._profile = []                                  # event hooks requested: the Python schedule
        u_d, i_d, uts_d = (torch.from_numpy(x).to(DEV) for x in (users, items, uts))
        assert model._native_l2_ok(i_d, None, False) == native
        got = model.forward_users(u_d, i_d, uts_d)
        torch.cuda.synchronize()
        assert any(t is not None for t in model._ka_flash_ws.values()), "the flash form of key addressing was expected"
        assert any(t is not None for t in model._fold_ws.values()), "the folded-tail form was expected"
        assert model._fold_for(model._enc_for_l2(n_parents=B)), "the folded tail over per-entity aggregates was expected"
        outs.append(got)
    a, b = outs
    assert bool(torch.isfinite(a.scores).all())
    assert torch.equal(a.user_o, b.user_o), "user_o"
    assert torch.equal(a.item_embeddings, b.item_embeddings), "item_embeddings"
    assert torch.equal(a.scores, b.scores), "scores"


def test_other_dims_keep_the_general_kernel(hip_lib):
    """Dim 16 / 128 mvin_project_relations and the dim-32 folded tables are linear_mfma_kernel's, as before (and the transposed
    copies of R_KGE they are built from stay in the workspace)."""
    rng = np.random.default_rng(7)
    n_entity, nR = 211, 3
    for dim in (16, 128):
        E, R, w = rnd(rng, n_entity, dim), rnd(rng, nR, dim, dim), rnd(rng, dim)
        n = hip_lib.mvin_project_relations_elems(n_entity, nR, dim)
        buf, ws = poisoned(n)
        ops.project_relations(E, R, w, out=ws)
        torch.cuda.synchronize()
        tab = n_entity * dim
        for r in range(nR):
            assert torch.equal(ws[r * tab:(r + 1) * tab].view(n_entity, dim), ops.linear([E], R[r].t().contiguous(), dim)), f"ER[{r}] dim {dim}"
        RT = ws[nR * tab + ((n_entity + 3) & ~3):].view(nR, dim, dim)
        assert torch.equal(RT, R.transpose(1, 2)), f"transposed R_KGE, dim {dim}"
        assert untouched(buf[n:])
    dim, K, nR = 32, 16, 5
    E = rnd(rng, n_entity, dim)
    enc_e, enc_r, p = fold_inputs(rng, n_entity, K, nR, dim)
    n = hip_lib.mvin_fold_tables_elems(n_entity, dim)
    buf, ws = poisoned(n)
    run_fold(E, enc_e, enc_r, rnd(rng, nR), p, K, nR, ws, True)
    torch.cuda.synchronize()
    tab = n_entity * dim
    Wstack = ws[6 * tab:6 * tab + 4 * dim * dim].view(4, dim, dim).clone()
    for i in range(4):
        assert torch.equal(ws[i * tab:(i + 1) * tab].view(n_entity, dim), ops.linear([E], Wstack[i], dim)), f"dim-32 folded table {i}"
    check_fold_block(ws[6 * tab:], p, 1.0 / K, dim)
    assert bool(torch.isfinite(ws[4 * tab:6 * tab]).all()) and untouched(buf[n:])
