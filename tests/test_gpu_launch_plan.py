"""-m gpu: the launchers whose persistent grid comes from the shared occupancy cache (mvin_amd/csrc/mvin_launch.h), across a change of
the relation count inside one process.  Their LDS grows with the relation count, so shape A, then shape B, then shape A again walks
the cache from one key to another and back: the two A results must be the same bits, and every result must agree with the oracle of
the kernel's own module, to that module's tolerance (the builders and references are theirs).  A grid of the wrong size still
computes the right answer -- the keying itself is pinned by tests/test_launch_plan_host.py; this module pins that the launchers
still run and still compute what they did at both ends of a change.  And, with two devices, the two launchers that used to grant
their LDS once per thread, on one device after the other."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_flash as flash_mod
import test_gpu_fold_f64 as f64
from mvin_amd import ops, synth
from parity import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NR_A, NR_B = 9, 200
N_ENTITY, B = 300, 100          # seven batches of 16 pairs, the last one short


def _aba(run, nr_b=NR_B):
    """run(nR) -> the launch's outputs, checked against its oracle inside.  A, B, A: the second A gives the first one's bits."""
    first, _, again = run(NR_A), run(nr_b), run(NR_A)
    for x, y in zip(first, again):
        assert torch.equal(x, y), "shape A differs after shape B ran in between"


def _l2_case(D, K, nR):
    w = f64._world(D, K, N_ENTITY, nR, "counts")
    c = f64._case(w, "stride", B, True, False, seed=3)
    t0, t1 = f64._logits(w, "unit")
    return w, c, t0, t1, f64._enc(w)


def _check_l2(w, c, t0, t1, got, K):
    _, b1, b2, a0, _, _ = w.bias
    r0, r1 = bench.l2_reference_f64(w.E, w.ae, w.ar, c.items, t0, t1, w.W1, w.W2, b1, b2, c.q, w.A0, a0, K)
    assert_close(got[0].cpu().numpy(), r0.cpu().numpy(), "nagg0 vs float64", rtol=1e-5, atol=2e-6)      # (test_gpu_prj.py's bounds)
    assert_close(got[1].cpu().numpy(), r1.cpu().numpy(), "nagg1 vs float64", rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("K", [16, 32])
def test_wave_per_parent_kernel_across_relation_counts(K, hip_lib):
    """mvin_gather_attn_l2_prj_ordered_fwd at D = 64 (mvin_fused_wpp.hip), parents in key order."""
    D = 64
    assert ops.gather_attn_l2_wpp_supported(D, K)

    def run(nR):
        w, c, t0, t1, (enc_e, enc_r, _) = _l2_case(D, K, nR)
        _, b1, b2, a0, _, _ = w.bias
        ws = ops.project_tables(w.E, w.W1, w.W2, b1, b2, w.A0, a0, K, True)
        got = ops.gather_attn_l2_prj(ws, enc_e, enc_r, c.items, t0, t1, c.q, B, 1, K, D, nR, N_ENTITY, order=ops.order_by_key(c.items))
        torch.cuda.synchronize()
        _check_l2(w, c, t0, t1, got, K)
        return got
    _aba(run)


def test_entity_aggregates_form_across_relation_counts(hip_lib):
    """mvin_gather_attn_l2_agg_fwd at K = 16 (mvin_fused_agg.hip)."""
    D, K = 64, 16

    def run(nR):
        assert ops.gather_attn_l2_agg_supported(D, K, N_ENTITY, nR)
        w, c, t0, t1, (enc_e, enc_r, _) = _l2_case(D, K, nR)
        _, b1, b2, a0, _, _ = w.bias
        ws = ops.project_tables(w.E, w.W1, w.W2, b1, b2, w.A0, a0, K, True)
        agg = ops.entity_aggregates(ws, enc_e, enc_r, t0, K, D, nR, N_ENTITY)
        got = ops.gather_attn_l2_agg(ws, agg, enc_e, enc_r, c.items, t0, t1, c.q, B, 1, K, D, nR, N_ENTITY)
        torch.cuda.synchronize()
        _check_l2(w, c, t0, t1, got, K)
        return got
    _aba(run)


@pytest.mark.parametrize("D", [64, 32])
def test_folded_score_kernel_across_relation_counts(D, hip_lib):
    """mvin_score_l2_folded_fwd at K = 16 (dim 64: mvin_fused_agg.hip, dim 32: mvin_fused_agg32.hip): the rule of test_gpu_fold_f64.py."""
    K = 16
    fid = "fold-D%dK%d" % (D, K)

    def run(nR):
        w, c, t0, t1, _ = _l2_case(D, K, nR)
        ws = f64._tables(w, "fold", t0, True)
        got = f64._launch(w, "fold", ws, c.items, t0, t1, c.q, c.uo, True)
        fails = []
        f64._compare(fid, f"{fid} nR={nR}", got, f64._references(w, c, t0, t1, True), fails)
        assert not fails, "\n".join(fails)
        return got
    _aba(run)


def test_dim32_wave_per_parent_kernel_across_relation_counts(hip_lib):
    """mvin_gather_attn_l2_fwd at D = 32, K = 8 (mvin_fused_d32.hip): inputs and bound of test_gpu_roofline_launch.py."""
    D, K = 32, 8
    assert ops.gather_attn_l2_variant(D, K, B, N_ENTITY) == 4

    def run(nR):
        g = torch.Generator(device=DEV)
        g.manual_seed(nR)
        table = torch.rand((N_ENTITY, D), device=DEV, generator=g) - 0.5
        adj_e = torch.randint(0, N_ENTITY, (N_ENTITY, K), device=DEV, generator=g, dtype=torch.int32)
        adj_r = torch.randint(0, nR, (N_ENTITY, K), device=DEV, generator=g, dtype=torch.int32)
        parents = torch.randint(0, N_ENTITY, (B,), device=DEV, generator=g, dtype=torch.int32)
        t0, t1 = torch.rand(nR, device=DEV, generator=g), torch.rand(nR, device=DEV, generator=g)
        W = (torch.rand((3, D, D), device=DEV, generator=g) - 0.5) / D ** 0.5
        q = torch.rand((B, D), device=DEV, generator=g)
        b = torch.rand((3, D), device=DEV, generator=g) - 0.5
        args = (table, adj_e, adj_r, parents, t0, t1, W[0], W[1], b[0], b[1], q, W[2], b[2])
        out = ops.gather_attn_l2(*args, B, 1, K, D, nR)
        torch.cuda.synchronize()
        max_abs, worst, ok = bench.check_l2_launch(out, *args, K, n_check=B)
        assert ok, (nR, max_abs, worst)
        return out[:2]
    _aba(run)


def _key_addressing_inputs(D, P, Nm, nR, has_set, n_user=40):
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * D + 10 * nR + P)
    rnd = lambda *s: torch.rand(s, device=DEV, generator=g) - 0.5     # noqa: E731
    E, R = rnd(N_ENTITY, D), rnd(nR, D, D) * 0.5
    w = rnd(D) if has_set else None
    n_o = P + (1 if has_set else 0)
    W, b = rnd(n_o * D, D) * 0.3, rnd(D)
    uts = torch.from_numpy(synth.ripple_sets(n_user, N_ENTITY, nR, P, Nm, seed=nR)).to(DEV)
    users = torch.randint(0, n_user, (B,), device=DEV, generator=g)
    items = torch.randint(0, N_ENTITY, (B,), device=DEV, generator=g)
    return E, R, w, W, b, uts, users, items, n_o, n_user


@pytest.mark.parametrize("P", [1, 2])
def test_flash_key_addressing_across_relation_counts(P, hip_lib):
    """mvin_key_addressing_flash_fwd with one and two hops: reference and bound of test_gpu_flash.py."""
    D, Nm = 64, 16

    def run(nR):
        assert ops.key_addressing_flash_supported(D, P, Nm, nR, N_ENTITY)
        E, R, w, W, b, uts, users, items, n_o, n_user = _key_addressing_inputs(D, P, Nm, nR, True)
        rec = ops.build_user_records(uts, P, nR, N_ENTITY)
        groups = ops.group_pairs_by_user(users, n_user=n_user)
        tabs = ops.key_addressing_flash_prepare(E, R, w, W, P)
        user_o = torch.full((B, D), float("nan"), device=DEV)
        ops.key_addressing_flash(E, tabs, rec, groups, items, P, Nm, nR, True, b, n_user, out=user_o)
        torch.cuda.synchronize()
        idx = torch.arange(B, device=DEV)
        _, ref_uo = flash_mod.reference_f64(E, R, w, W, b, uts, users, items, P, Nm, True, idx)
        assert_close(user_o.cpu().numpy(), ref_uo.cpu().numpy(), "user_o vs float64", rtol=1e-5, atol=2e-6)
        return (user_o,)
    _aba(run)


@pytest.mark.parametrize("D,nr_b", [(16, 39), (64, NR_B)], ids=["d16-wave", "d64-dense"])
def test_grouped_key_addressing_across_relation_counts(D, nr_b, hip_lib):
    """mvin_key_addressing_grouped_fwd at D = 16 (one wave per user, mvin_keyaddr_wave.hip: 39 relations are 75 KB of LDS, two workgroups
    per CU where 9 relations leave four; 200 would be past what that kernel takes) and at D = 64 (mvin_keyaddr_dense.hip), against the
    float64 reference of test_gpu_flash.py before the user MLP, at its bound."""
    P, Nm = 2, 16

    def run(nR):
        assert ops.key_addressing_grouped_supported(D, P, Nm, nR)
        E, R, w, W, b, uts, users, items, n_o, n_user = _key_addressing_inputs(D, P, Nm, nR, True)
        groups = ops.group_pairs_by_user(users, n_user=n_user)
        a = torch.full((B, n_o * D), float("nan"), device=DEV)
        ops.key_addressing_grouped(E, R, w, uts, groups, items, P, a, n_o * D, nR)
        torch.cuda.synchronize()
        ref_cat, _ = flash_mod.reference_f64(E, R, w, W, b, uts, users, items, P, Nm, True, torch.arange(B, device=DEV))
        assert_close(a.cpu().numpy(), ref_cat.cpu().numpy(), "o_list vs float64", rtol=1e-5, atol=2e-6)
        return (a,)
    _aba(run, nr_b)


TWO_DEVICES = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from mvin_amd import ops
D, B, n_entity = 64, 64, 300
rng = np.random.default_rng(7)
f = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32) * 0.3)      # noqa: E731
host = dict(E=f(n_entity, D), q=f(B, D), uo=f(B, D), n0=f(B, D), n1=f(B, D), W0=f(D, D), b0=f(D), A0=f(D, D), a0=f(D), A1=f(D, D), a1=f(D),
            Wmix=f(3 * D, D), bmix=f(D))
items = torch.from_numpy(rng.permutation(n_entity)[:B].astype(np.int64))            # distinct keys: one key per bucket, one possible order
assert ops.l2_tail_supported(D)
outs = []
for dev in (0, 1):
    torch.cuda.set_device(dev)
    t = {k: v.to("cuda:%d" % dev) for k, v in host.items()}
    it = items.to("cuda:%d" % dev)
    order = ops.order_by_key(it)
    tail = ops.l2_tail(t["E"], it, t["q"], t["uo"], t["n0"], t["n1"], t["W0"], t["b0"], t["A0"], t["a0"], t["A1"], t["a1"], t["Wmix"], t["bmix"])
    torch.cuda.synchronize()
    outs.append([order.cpu()] + [x.cpu() for x in tail if x is not None])
assert len(outs[0]) == len(outs[1]) >= 3
assert sorted(outs[0][0].tolist()) == list(range(B))
for x, y in zip(*outs):
    assert torch.isfinite(x.float()).all() and torch.equal(x, y), "device 0 and device 1 differ"
print("TWO DEVICES OK")
"""


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
def test_one_thread_drives_two_devices(tmp_path, hip_lib):
    """mvin_order_by_key and mvin_l2_tail_fwd in its FLASH form (l2_tail_flash_kernel, 96 KB of LDS: opt-in with MVIN_TAIL_FLASH=1, read once
    per process: hence the child) on device 0 and then on device 1 from one thread: the LDS grant belongs to each device's copy of the
    function.  Values: tests/test_gpu_tail.py."""
    script = tmp_path / "two_devices.py"
    script.write_text(TWO_DEVICES)
    env = dict(os.environ, MVIN_TAIL_FLASH="1")
    res = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "TWO DEVICES OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
