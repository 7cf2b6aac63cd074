"""The folded score forms AT the limits their _supported predicates promise (fold_applies / agg_applies / fold_gather_applies, mvin_l2_kernel_plan.h):
an entity table of 1 GiB - one row, an adjacency up to 1 GiB, B D 4 one row below 2^31 -- where the kernels' 32-bit buffer offsets, (int)
casts of table bytes and unsigned query-row offsets come closest to wrapping.  Every case is its own test so that a failure names its form.

Inputs come from a seeded torch.Generator on the device, tensors are freed between forms, the reference (tests/fold_ref.py, float64 on the
plain adjacency) is evaluated on sampled pairs / rows only.  A case skips only when torch.cuda.mem_get_info shows less free memory than
the peak stated in its docstring.  Tolerances: the rule of tests/test_gpu_fold_f64.py (err_hip <= 4 err_f32 + 2e-6 per output, err_f32 from
the fp32 evaluation of the same reference), plus the absolute bounds of the tail / aggregates tests where the case meets them.

The absolute bounds: asserted for sigmoid everywhere, for every output at dim 32 and for nagg0 | nagg1 of the aggregates form (_hold).  Item
embeddings and scores at dim 64 miss them at these magnitudes (weights normal x 0.3: |scores| up to 50) exactly as the fp32 reference does,
and keep the relative rule.

MEASURED on an MI355X (peak allocated, wall time of the case; then err_hip | err_f32 | err_hip / (4 err_f32 + 2e-6) | error / absolute bound):
    table-fold-D64K32    9.2 GiB 0.6 s   item_emb 1.2e-5 | 1.9e-5 | 0.16 | 3.66   scores 2.0e-5 | 2.2e-5 | 0.22 | 1.21   sigmoid 2.4e-6 | 2.7e-6 | 0.19 | 0.49
    table-gather-D64K32  9.2 GiB 0.3 s   item_emb 1.2e-5 | 1.9e-5 | 0.16 | 3.66   scores 1.8e-5 | 2.2e-5 | 0.20 | 1.38   sigmoid 2.8e-6 | 2.7e-6 | 0.22 | 0.52
    table-agg-D64K32     8.2 GiB 0.3 s   nagg0    3.8e-8 | 2.8e-8 | 0.02 | 0.02   nagg1  1.0e-7 | 7.3e-8 | 0.05 | 0.03
    table-fold-D32K16    9.2 GiB 0.4 s   item_emb 3.6e-6 | 3.8e-6 | 0.21 | 0.65   scores 4.0e-6 | 4.0e-6 | 0.22 | 0.51   sigmoid 8.6e-7 | 6.5e-7 | 0.19 | 0.16
    table-fold-D64K64   11.2 GiB 0.3 s   item_emb 1.5e-5 | 1.5e-5 | 0.24 | 2.96   scores 2.4e-5 | 2.4e-5 | 0.25 | 1.46   sigmoid 2.2e-6 | 4.7e-6 | 0.11 | 0.53
    batch-fold-D64K16   10.5 GiB 0.5 s   item_emb 1.7e-5 | 2.1e-5 | 0.19 | 3.45   scores 2.4e-5 | 2.1e-5 | 0.28 | 1.87   sigmoid 2.7e-6 | 2.5e-6 | 0.22 | 0.55
    batch-gather-D64K16 12.5 GiB 0.4 s   item_emb 1.7e-5 | 2.1e-5 | 0.19 | 3.55   scores 2.2e-5 | 2.1e-5 | 0.26 | 2.20   sigmoid 3.2e-6 | 2.5e-6 | 0.26 | 0.50
    batch-fold-D32K16   12.7 GiB 0.2 s   item_emb 2.5e-6 | 4.0e-6 | 0.14 | 0.59   scores 2.7e-6 | 4.5e-6 | 0.13 | 0.39   sigmoid 5.7e-7 | 4.6e-7 | 0.15 | 0.15
Every table (TA1 | TA2 | T0A | M0 | H0 | G, S0 | G) met rtol 2e-5 / atol 5e-6 on its last 16 and 256 sampled rows; no limit had to be tightened.
Run with -s for the figures of a run (lines starting with MEASURED).
"""
import time
import types

import pytest
import torch

from fold_ref import aggregates_reference, compare, fold_reference, fold_tables_reference, report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GIB = 1 << 30
STATS = {}
OUTPUTS = ("item_emb", "scores", "sigmoid")


def _hold(D, names):
    """Which outputs are held to the absolute bounds against float64 (fold_ref.TAIL_BOUNDS) besides the relative rule: see the docstring."""
    return [D == 32 or n in ("sigmoid", "nagg0", "nagg1") for n in names]


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, the case peaks at {gib} GiB")
    torch.cuda.reset_peak_memory_stats()


def _done(name, t_start):
    torch.cuda.synchronize()
    print(f"MEASURED {name}: peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB, wall {time.perf_counter() - t_start:.2f} s")
    report(STATS, name)
    torch.cuda.empty_cache()


def _world(D, K, n_entity, nR, seed, force=True):
    """E, the plain and the encoded adjacency, the parameters.  Random slots; every other row repeats its first half in its second; the rows
    of the last 64 entities and of 64 chosen parents have children n_entity - 1 and n_entity - 2 (the table's last rows, twice)."""
    from mvin_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    f = lambda *s: torch.randn(*s, device=DEV, generator=g).mul_(0.3)      # noqa: E731
    w = types.SimpleNamespace(D=D, K=K, n_entity=n_entity, nR=nR, g=g, f=f)
    w.E = f(n_entity, D)
    w.ae = torch.randint(0, n_entity, (n_entity, K), device=DEV, generator=g, dtype=torch.int32)
    w.ar = torch.randint(0, nR, (n_entity, K), device=DEV, generator=g, dtype=torch.int32)
    w.ae[::2, K // 2:] = w.ae[::2, : K // 2]
    w.ar[::2, K // 2:] = w.ar[::2, : K // 2]
    w.chosen = torch.randint(64, max(65, n_entity - 64), (64,), device=DEV, generator=g)
    if force:
        for rows in (torch.arange(max(0, n_entity - 64), n_entity, device=DEV), w.chosen):
            w.ae[rows, 0], w.ae[rows, 1], w.ae[rows, K - 1] = n_entity - 1, n_entity - 2, n_entity - 1
    w.enc_e, w.enc_r, _ = ops.encode_adjacency(w.ae, w.ar)
    w.W0, w.W1, w.W2, w.A0, w.A1, w.Wmix = f(D, D), f(D, D), f(D, D), f(D, D), f(D, D), f(3 * D, D)
    w.b0, w.b1, w.b2, w.a0, w.a1, w.bmix = (f(D) for _ in range(6))
    w.t0, w.t1 = f(nR), f(nR)
    return w


def _table_batch(w, B=4096):
    """B items: 64 at the very end of the table, 64 at its start, the 64 forced parents, the rest random; the pairs to check: those 192
    and 256 sampled ones."""
    n = w.n_entity
    items = torch.randint(0, n, (B,), device=DEV, generator=w.g)
    items[:64] = torch.arange(n - 64, n, device=DEV)
    items[64:128] = torch.arange(0, 64, device=DEV)
    items[128:192] = w.chosen
    pick = torch.cat([torch.arange(192, device=DEV), 192 + torch.randperm(B - 192, device=DEV, generator=w.g)[:256]])
    return items, w.f(B, w.D), w.f(B, w.D), pick


def _sample_rows(w):
    """The table's last 16 rows plus 256 sampled ones."""
    n = w.n_entity
    return torch.cat([torch.arange(n - 16, n, device=DEV), torch.randint(0, n, (256,), device=DEV, generator=w.g)])


def _reference(w, items, q, uo, pick):
    args = (w.E, w.ae, w.ar, items[pick], w.t0, w.t1, q[pick], uo[pick], w.W0, w.b0, w.W1, w.b1, w.W2, w.b2, w.A0, w.a0, w.A1, w.a1, w.Wmix, w.bmix, w.K)
    return fold_reference(*args), fold_reference(*args, dtype=torch.float32)


def _fold_tables(w, aggregates=True, out=None):
    from mvin_amd import ops
    return ops.fold_tables(w.E, w.enc_e, w.enc_r, w.t0, w.W0, w.b0, w.W1, w.b1, w.W2, w.b2, w.A0, w.a0, w.Wmix, w.bmix, w.A1, w.K, w.nR, out=out,
                           aggregates=aggregates)


def _check_fold_tables(name, w, ws, aggregates, fails):
    rows = _sample_rows(w)
    ref = fold_tables_reference(w.E, w.ae, w.ar, w.t0, w.W0, w.W1, w.W2, w.A0, w.Wmix, w.K, rows=rows)
    T = ws[: 6 * w.n_entity * w.D].view(6, w.n_entity, w.D)
    for i, nm in enumerate(["TA1", "TA2", "T0A", "M0"] + (["H0", "G"] if aggregates else [])):
        err = (T[i][rows].double() - ref[nm]).abs()
        worst = float((err / (2e-5 * ref[nm].abs() + 5e-6)).max())
        if not worst <= 1.0:
            fails.append(f"{name} table {nm}: {worst:.2f} x (rtol 2e-5, atol 5e-6), max abs err {float(err.max()):.3e}")


def _score(w, form, ws, items, q, uo, order=None):
    from mvin_amd import ops
    if form == "fold":
        out = ops.score_l2_folded(ws, w.enc_e, w.enc_r, items, w.t0, w.t1, q, uo, w.A1, w.a1, w.Wmix, w.K, w.D, w.nR, w.n_entity)
    else:
        out = ops.score_l2_folded_gather(ws, w.enc_e, w.enc_r, items, w.t0, w.t1, q, uo, w.A1, w.a1, w.Wmix, w.K, w.D, w.nR, w.n_entity, order=order)
    torch.cuda.synchronize()
    return out


def _largest_table(name, form, D, K, n_entity, peak_gib, seed):
    from mvin_amd import ops
    _need(peak_gib)
    t_start = time.perf_counter()
    nR = 9
    queries = [ops.score_l2_folded_supported] + ([ops.score_l2_folded_gather_supported, ops.gather_attn_l2_agg_supported] if D == 64 and K < 64 else [])
    for supported in queries:
        assert supported(D, K, n_entity, nR) and not supported(D, K, n_entity + 1, nR), supported.__name__
    w = _world(D, K, n_entity, nR, seed)
    items, q, uo, pick = _table_batch(w)
    ref64, ref32 = _reference(w, items, q, uo, pick)
    fails = []
    if form == "aggregates":
        pt = ops.project_tables(w.E, w.W1, w.W2, w.b1, w.b2, w.A0, w.a0, K, True)
        agg = ops.entity_aggregates(pt, w.enc_e, w.enc_r, w.t0, K, D, nR, n_entity)
        rows = _sample_rows(w)
        ref = aggregates_reference(w.E, w.ae, w.ar, w.t0, w.W1, w.W2, w.A0, K, rows=rows)
        for i, nm in enumerate(("S0", "G")):
            err = (agg.view(2, n_entity, D)[i][rows].double() - ref[nm]).abs()
            worst = float((err / (2e-5 * ref[nm].abs() + 5e-6)).max())
            if not worst <= 1.0:
                fails.append(f"{name} table {nm}: {worst:.2f} x (rtol 2e-5, atol 5e-6), max abs err {float(err.max()):.3e}")
        for oname, order in (("as given", None), ("key order", ops.order_by_key(items))):
            got = ops.gather_attn_l2_agg(pt, agg, w.enc_e, w.enc_r, items, w.t0, w.t1, q, items.shape[0], 1, K, D, nR, n_entity, order=order)
            torch.cuda.synchronize()
            compare(("nagg0", "nagg1"), [g[pick] for g in got], ref64[:2], ref32[:2], f"{name} order={oname}", fails, _hold(D, ("nagg0", "nagg1")), STATS, name)
        del pt, agg
    else:
        ws = _fold_tables(w, aggregates=form == "fold")
        _check_fold_tables(name, w, ws, form == "fold", fails)
        orders = (("as given", None),) if form == "fold" else (("as given", None), ("key order", ops.order_by_key(items)))
        for oname, order in orders:
            got = _score(w, form, ws, items, q, uo, order)
            compare(OUTPUTS, [g[pick] for g in got], ref64[2:], ref32[2:], f"{name} order={oname}", fails,
                    _hold(D, OUTPUTS), STATS, name)
        del ws
    del w, items, q, uo, got
    _done(name, t_start)
    assert not fails, "\n".join(fails)


def test_largest_table_dim64_folded(hip_lib):
    """D = 64, K = 32, n_entity = 4 194 303 (table = 1 GiB - 256 B): mvin_fold_tables -> mvin_score_l2_folded_fwd.  Peak 10 GiB."""
    _largest_table("table-fold-D64K32", "fold", 64, 32, 4194303, 10, seed=11)


def test_largest_table_dim64_folded_gather(hip_lib):
    """The same table: mvin_fold_tables_ex(aggregates = 0) -> mvin_score_l2_folded_gather_fwd, pairs as given and in key order.  Peak 10 GiB."""
    _largest_table("table-gather-D64K32", "gather", 64, 32, 4194303, 10, seed=11)


def test_largest_table_dim64_aggregates(hip_lib):
    """The same table: mvin_project_tables -> mvin_entity_aggregates -> mvin_gather_attn_l2_agg_fwd, S0 | G and nagg0 | nagg1.  Peak 9 GiB."""
    _largest_table("table-agg-D64K32", "aggregates", 64, 32, 4194303, 9, seed=11)


def test_largest_table_dim32_folded(hip_lib):
    """D = 32, K = 16, n_entity = 8 388 607 (table = 1 GiB - 128 B): the folded form of mvin_fused_agg32.hip.  Peak 10 GiB."""
    _largest_table("table-fold-D32K16", "fold", 32, 16, 8388607, 10, seed=12)


def test_largest_table_fanout64_folded(hip_lib):
    """D = 64, K = 64, n_entity = 4 194 303: an adjacency of 1 GiB - 256 B beside the 1 GiB table, folded form.  Peak 12 GiB."""
    _largest_table("table-fold-D64K64", "fold", 64, 64, 4194303, 12, seed=13)


def _largest_batch(name, form, D, K, B, peak_gib, seed):
    """n_entity = 603, B D 4 one row below 2^31: all outputs finite; the first 64, last 64 and 256 sampled pairs against the reference."""
    from mvin_amd import ops
    _need(peak_gib)
    t_start = time.perf_counter()
    n_entity, nR = 603, 9
    supported = ops.score_l2_folded_supported if form == "fold" else ops.score_l2_folded_gather_supported
    assert supported(D, K, n_entity, nR) and (B + 1) * D * 4 == 1 << 31
    w = _world(D, K, n_entity, nR, seed, force=False)
    items = torch.randint(0, n_entity, (B,), device=DEV, generator=w.g)
    q, uo = w.f(B, D), w.f(B, D)
    pick = torch.cat([torch.arange(64, device=DEV), torch.arange(B - 64, B, device=DEV), torch.randint(64, B - 64, (256,), device=DEV, generator=w.g)])
    ref64, ref32 = _reference(w, items, q, uo, pick)
    fails = []
    ws = _fold_tables(w, aggregates=form == "fold")
    got = _score(w, form, ws, items, q, uo)
    for nm, g in zip(("item_emb", "scores", "sigmoid"), got):
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{name} {nm}: not finite everywhere")
    compare(OUTPUTS, [g[pick] for g in got], ref64[2:], ref32[2:], name, fails, _hold(D, OUTPUTS), STATS, name)
    from mvin_amd._lib import MvinHipError
    with pytest.raises(MvinHipError):                         # one pair more: B D 4 = 2^31, refused
        big = torch.empty((B + 1, D), device=DEV)
        _score(w, form, ws, torch.zeros(B + 1, dtype=torch.int64, device=DEV), big, big)
    del w, ws, items, q, uo, got
    _done(name, t_start)
    assert not fails, "\n".join(fails)


def test_largest_batch_dim64_folded(hip_lib):
    """D = 64, K = 16, B = 2^23 - 1: mvin_score_l2_folded_fwd.  Peak 11 GiB (q, user_o, item_emb: 2 GiB each)."""
    _largest_batch("batch-fold-D64K16", "fold", 64, 16, (1 << 23) - 1, 11, seed=21)


def test_largest_batch_dim64_folded_gather(hip_lib):
    """D = 64, K = 16, B = 2^23 - 1: mvin_score_l2_folded_gather_fwd.  Peak 13 GiB."""
    _largest_batch("batch-gather-D64K16", "gather", 64, 16, (1 << 23) - 1, 13, seed=21)


def test_largest_batch_dim32_folded(hip_lib):
    """D = 32, K = 16, B = 2^24 - 1: the folded form of mvin_fused_agg32.hip.  Peak 13 GiB."""
    _largest_batch("batch-fold-D32K16", "fold", 32, 16, (1 << 24) - 1, 13, seed=22)
