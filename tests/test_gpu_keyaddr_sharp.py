"""-m gpu: every key-addressing softmax of the library against float64 at TRAINED logit scales.

The user side of a score (MVIN._key_addressing, model.py:161-240) is computed in nine places, each with a softmax of its own: the streaming
per-pair kernel (mvin_keyaddr_stream.hip: online softmax), the register-resident per-pair kernel (mvin_keyaddr.hip), the general fallback
(mvin_ripple_attn_fwd), the wave-per-user kernels of dim 16 / 32 (mvin_keyaddr_wave.hip), the dense grouped kernel (mvin_keyaddr_dense.hip:
lane groups merged through exp(mx - M), padding rows at -inf), the kernel over static per-user records and its gathered form
(mvin_keyaddr_static.hip: chunked online softmax) and the flash form (mvin_keyaddr_flash.hip, which returns user_o).  Their own modules feed
them near-uniform logits (standard deviation 0.8 .. 2), where every rescale factor is 1 to three digits, nothing underflows and no row has a
winner.  Here each form is called directly through ``ops`` -- chosen by its shape, the choice asserted through the exported predicates -- on
the six logit regimes of tests/keyaddr_ref.py (unit: the control; sharp; planted; ascending; descending; offset), each of which asserts its own
condition in float64 on the reference's logits before anything is compared.

For every (form, regime, shape): the output buffer starts as NaN and ends finite; two launches give the same bits; per output
err_hip = max |kernel - float64| <= 4 err_f32 + 2e-6 (the project's rule, parity.check_case / test_gpu_fold_f64.py), err_f32 the fp32
evaluation of the SAME reference in the association orders the kernels use, over at least 256 pairs of which the case's are the first B --
never the code under test; in the unit regime also the bound of the form's own module against float64 (rtol 2e-5 / atol 2e-6 per pair,
rtol 1e-5 / atol 2e-6 grouped and flash).  planted, forms that return o-vectors: every o-vector equals the planted tail row E[t*] within
4 ulp per element -- all other weights are below Nm e^-39, what remains is one rounding in 1/z, one in the product and the accumulation of
exact zeros; this is the assertion that sees a weight on the wrong slot.  Across forms: dense / static / gathered on one hand, flash against
dense + mvin_linear_fwd on the other agree within the sum of their two bounds.

The flash form's user_o is sum_m p_m (E[t_m] . W_j): its per-call TW tables hold the user MLP applied per entity.  That order is part of its
yardstick (keyaddr_ref.yardstick(tw=True)) and of no other form's.

MEASURED on an MI355X, the case with the worst ratio per (form, regime): err_hip | err_f32 | err_hip / (4 err_f32 + 2e-6); o-vectors, for flash
user_o.  No form missed the rule in any regime; in planted every o-vector of every form was the tail row itself, bit for bit.
    form       unit                          sharp                         planted                       ascending                     descending                    offset
    stream     1.1e-06 | 1.3e-06 | 0.15      2.1e-05 | 3.6e-05 | 0.14      0.0e+00 | 0.0e+00 | 0.00      7.6e-07 | 6.2e-07 | 0.17      1.0e-06 | 8.1e-07 | 0.20      9.8e-07 | 5.0e-07 | 0.24
    register   3.8e-07 | 8.7e-07 | 0.07      2.0e-05 | 3.3e-05 | 0.15      0.0e+00 | 0.0e+00 | 0.00      7.1e-07 | 1.0e-06 | 0.12      2.4e-05 | 6.5e-05 | 0.09      6.7e-07 | 6.2e-07 | 0.15
    users_feed 1.0e-07 | 1.5e-07 | 0.04      1.8e-05 | 3.7e-05 | 0.12      0.0e+00 | 0.0e+00 | 0.00      3.0e-06 | 3.5e-06 | 0.19      3.7e-06 | 3.4e-06 | 0.23      9.2e-07 | 6.9e-07 | 0.19
    general    9.8e-07 | 1.0e-06 | 0.16      3.3e-05 | 4.8e-05 | 0.17      0.0e+00 | 0.0e+00 | 0.00      1.4e-05 | 3.0e-05 | 0.12      2.4e-05 | 2.8e-05 | 0.21      9.8e-07 | 7.3e-07 | 0.20
    wave       7.1e-08 | 7.4e-08 | 0.03      4.0e-05 | 3.0e-05 | 0.33      0.0e+00 | 0.0e+00 | 0.00      6.1e-06 | 3.7e-06 | 0.36      7.7e-06 | 3.8e-06 | 0.45      2.1e-06 | 9.2e-07 | 0.38
    dense      9.3e-07 | 5.6e-07 | 0.22      1.0e-04 | 4.4e-05 | 0.57      0.0e+00 | 0.0e+00 | 0.00      1.1e-05 | 3.1e-06 | 0.80      9.3e-06 | 2.6e-06 | 0.74      1.6e-06 | 4.6e-07 | 0.41
    static     4.4e-07 | 1.9e-07 | 0.16      8.5e-05 | 3.5e-05 | 0.59      0.0e+00 | 0.0e+00 | 0.00      9.2e-06 | 3.6e-06 | 0.56      1.2e-05 | 3.6e-06 | 0.71      1.7e-06 | 6.9e-07 | 0.35
    er         2.9e-07 | 1.5e-07 | 0.11      5.8e-05 | 3.4e-05 | 0.42      0.0e+00 | 0.0e+00 | 0.00      1.1e-05 | 3.6e-06 | 0.67      1.0e-05 | 3.6e-06 | 0.63      1.5e-06 | 7.3e-07 | 0.32
    flash      7.1e-07 | 2.6e-07 | 0.23      4.7e-05 | 2.5e-05 | 0.46      4.0e-06 | 7.7e-06 | 0.12      1.0e-05 | 4.1e-06 | 0.57      1.1e-05 | 3.9e-06 | 0.61      2.9e-06 | 2.8e-06 | 0.22
Run with -s for the figures of a run (lines starting with MEASURED).  54 cases, 26 s.

That the module bites was checked on scratch copies of the kernels.  With the streaming kernel's online rescale (sc = expf(ms - mx)) replaced
by 1 the stream / users_feed cases fail in every regime but descending, where no rescale is ever taken: err_hip up to 1.0 in ascending, 5.4 in
sharp, 15 in planted.  test_gpu_keyaddr.py sees that fault too (its logits' standard deviation of 2 is enough for this one: 0.16 .. 1.5 off).
With two slots' hop weights swapped in that kernel, planted names the o-vectors that are not their tail row (5 .. 74 per shape, 3e-2 .. 1e-1 off).
"""
import functools

import pytest
import torch

import keyaddr_ref as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORMS = list(kr.CASES)
PER_PAIR = {"stream", "register", "users_feed", "general"}
UNIT_BOUND = {f: ((2e-5, 2e-6) if f in PER_PAIR else (1e-5, 2e-6)) for f in FORMS}
ULP = 2.0 ** -23
STATS = {}
_OUT = {}


def _key(c):
    return tuple(sorted(c.items()))


@functools.lru_cache(maxsize=None)
def _world(regime, key):
    """Inputs of one (regime, shape), their float64 reference over all pairs and the regime's condition: built once, left unchanged."""
    inp = kr.build_inputs(regime, device=DEV, **dict(key))
    ref = kr.reference(inp)
    kr.condition(inp, ref)
    return inp, ref


@functools.lru_cache(maxsize=None)
def _yard(regime, key, tw):
    inp, ref = _world(regime, key)
    return kr.yardstick(inp, ref, tw=tw)


def _twice(launch, shape):
    """Run ``launch(out)`` twice on NaN-filled buffers: every row written, the same bits."""
    first = None
    for _ in range(2):
        out = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        launch(out)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), "rows left unwritten (or not finite)"
        if first is None:
            first = out
    assert torch.equal(first, out), "two launches differ"
    return out


def _per_pair_feed(inp, B):
    sel = inp.uts[inp.users[:B]]                              # [B, P, 3, Nm]
    mk = lambda x: [sel[:, j, x].contiguous() for j in range(sel.shape[1])]      # noqa: E731
    # V[b, r, :] = E[item_b] . R_KGE[r]: the caller's part of mvin_key_addressing_fwd's contract, formed in float64
    V = torch.einsum("bi,rij->brj", inp.E[inp.items[:B]].double(), inp.R.double()).float().contiguous()
    return mk(0), mk(1), mk(2), V


def _run(form, regime, c):
    """-> (o [B, n_o, D] or None, user_o [B, D] or None) of one form on one case; cached, so that forms that share a case meet on it."""
    from mvin_amd import ops
    k = (form, regime, _key(c))
    if k in _OUT:
        return _OUT[k]
    inp, _ = _world(regime, _key(c))
    D, Nm, P, nR, B, nE = inp.D, inp.Nm, inp.P, inp.nR, c["n_pairs"], inp.n_entity
    n_o = P + (1 if inp.has_set else 0)
    ldo = n_o * D
    o = uo = None
    stream_shape = P >= 1 and Nm <= 64 and nR * D * 4 <= 3072        # include/mvin_hip.h: what the streaming pipeline takes
    if form in ("stream", "register", "users_feed"):
        assert stream_shape == (form != "register")
        if form == "register":
            assert ops.key_addressing_supported(Nm, D)
        mh, mr, mt, V = _per_pair_feed(inp, B)
        o = _twice(lambda out: ops.key_addressing(inp.E_table, V, inp.w, mh, mr, mt, P, out, ldo, nR), (B, ldo))
        if form == "users_feed":
            for dt in (torch.int64, torch.int32):
                u = _twice(lambda out: ops.key_addressing_users(inp.E_table, V, inp.w, inp.uts, inp.users[:B].to(dt), P, out, ldo, nR), (B, ldo))
                assert torch.equal(u, o), "users feed and per-pair arrays differ"
    elif form == "general":
        assert P == 1 and inp.has_set
        mh, mr, mt, V = _per_pair_feed(inp, B)

        def launch(out):
            ops.ripple_attn(inp.E_table, mh[0], None, mh[0], None, inp.w, 1, out, 0, ldo, nR)
            ops.ripple_attn(inp.E_table, mh[0], mr[0], mt[0], V, None, 0, out, D, ldo, nR)
        o = _twice(launch, (B, ldo))
    else:
        users, items = inp.users[:B].contiguous(), inp.items[:B].contiguous()
        groups = ops.group_pairs_by_user(users, n_user=inp.n_user)
        assert ops.key_addressing_grouped_supported(D, P, Nm, nR)
        kw = {}
        if form in ("static", "er", "flash"):
            assert ops.user_records_len(P, Nm, nR) > 0
            rec = ops.build_user_records(inp.uts, P, nR, nE)
        if form in ("static", "er"):
            assert ops.user_records_supported(D, P, Nm, nR)
            kw["records"] = rec
        if form == "er":
            assert ops.key_addressing_grouped_er_supported(D, P, Nm, nR, nE, inp.has_set)
            kw["er"] = ops.project_relations(inp.E, inp.R, inp.w)
        if form == "wave":
            assert D in (16, 32) and P in (1, 2) and Nm <= 64
        if form == "flash":
            assert ops.key_addressing_flash_supported(D, P, Nm, nR, nE)
            tabs = ops.key_addressing_flash_prepare(inp.E, inp.R, inp.w, inp.W_mlp, P)
            outs = [_twice(lambda out: ops.key_addressing_flash(inp.E, tabs, rec, groups, items.to(dt), P, Nm, nR, inp.has_set, inp.b_mlp,
                                                                inp.n_user, out=out), (B, D)) for dt in (torch.int64, torch.int32)]
            assert torch.equal(outs[0], outs[1]), "the two id widths differ"
            uo = outs[0]
        else:
            o = _twice(lambda out: ops.key_addressing_grouped(inp.E_table, inp.R, inp.w, inp.uts, groups, items, P, out, ldo, nR, **kw), (B, ldo))
    if o is not None:
        o = o.view(B, n_o, D)
    _OUT[k] = (o, uo)
    return o, uo


def _bound(regime, c, name, tw=False):
    return 4 * _yard(regime, _key(c), tw)[name] + 2e-6


def _compare(form, regime, c, o, uo, fails):
    inp, ref = _world(regime, _key(c))
    B = c["n_pairs"]
    what = f"{form} {regime} {kr.case_id(c)}"
    y = _yard(regime, _key(c), form == "flash")
    for name, got, r64 in (("o", o, ref.o[:B]), ("user_o", uo, ref.user_o[:B])):
        if got is None:
            continue
        err = (got.double() - r64).abs()
        err_hip, err_f32 = float(err.max()), y[name]
        rel = err_hip / (4 * err_f32 + 2e-6)
        s = STATS.setdefault((form, regime, name), [0.0, 0.0, 0.0])
        if rel >= s[2]:
            s[:] = [err_hip, err_f32, rel]
        if not rel <= 1.0:
            fails.append(f"{what} {name}: err_hip {err_hip:.3e} > 4 x err_f32 {err_f32:.3e} + 2e-6 ({rel:.2f} x)")
        if regime == "unit":
            rtol, atol = UNIT_BOUND[form]
            worst = float((err / (rtol * r64.abs() + atol)).max())
            if not worst <= 1.0:
                fails.append(f"{what} {name}: {worst:.2f} x the form's own bound (rtol {rtol:g}, atol {atol:g})")
    if regime == "planted" and o is not None:
        slots, tails = kr.planted_rows(inp, B)
        miss = (o.double() - tails.double()).abs() > 4 * ULP * tails.double().abs()
        if bool(miss.any()):
            b, j, _ = (int(x) for x in miss.nonzero()[0])
            fails.append(f"{what}: {int(miss.any(-1).sum())} o-vectors are not the planted tail row within 4 ulp; first: pair {b} block {j} "
                         f"planted slot {int(slots[b, j])}, max |o - E[t*]| {float((o[b, j] - tails[b, j]).abs().max()):.3e}")


@pytest.mark.parametrize("regime", kr.REGIMES)
@pytest.mark.parametrize("form", FORMS)
def test_form_against_float64(form, regime, hip_lib):
    from mvin_amd import ops
    fails = []
    for c in kr.CASES[form]:
        o, uo = _run(form, regime, c)
        _compare(form, regime, c, o, uo, fails)
        inp, _ = _world(regime, _key(c))
        # forms that take the same case agree within the sum of their bounds
        if form in ("static", "er") and not c["bf16"]:
            peer, _ = _run("dense", regime, c)
            d = float((o - peer).abs().max())
            if not d <= 2 * _bound(regime, c, "o"):
                fails.append(f"{form} {regime} {kr.case_id(c)}: {d:.3e} from the dense kernel, the two bounds add to {2 * _bound(regime, c, 'o'):.3e}")
        if form == "flash":
            peer, _ = _run("dense", regime, c)
            lin = ops.linear([peer.reshape(peer.shape[0], -1).contiguous()], inp.W_mlp, inp.D, bias=inp.b_mlp)
            d, tol = float((uo - lin).abs().max()), _bound(regime, c, "user_o", True) + _bound(regime, c, "user_o")
            if not d <= tol:
                fails.append(f"flash {regime} {kr.case_id(c)}: {d:.3e} from dense + linear, the two bounds add to {tol:.3e}")
    for (f, r, name), s in STATS.items():
        if (f, r) == (form, regime):
            print(f"MEASURED {f} {r} {name}: err_hip {s[0]:.3e} | err_f32 {s[1]:.3e} | {s[2]:.3f}")
    assert not fails, "\n".join(fails)
