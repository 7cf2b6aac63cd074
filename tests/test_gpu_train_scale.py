"""-m gpu: the whole training step at the batch sizes that are TIMED (bench.py --full, scripts/bench_train.py: 512 and
4 096 pairs, dim 64, fan-out up to 32), against oracle/train_ref.py run in FLOAT64: loss, every parameter gradient, no
gradient where the reference has none; then three applied steps, eager and as a replayed hipGraph.

tests/test_gpu_train.py compares with the float32 oracle at toy sizes, where that is harmless.  Here the float32 CPU
oracle alone is a visible share of the project's gradient tolerance away from float64, so the reference is the float64
route and the tolerance, per parameter, is the larger of
    2e-4 * max|g| + 1e-7                       (check_grads of test_gpu_train.py), and
    4 * max|g_float32_oracle - g_float64|      (both computed on the CPU inside the test).
The GPU sums the same float32 terms as the float32 oracle in another order (atomics, MFMA tiles): an error of the same
size, not a smaller one, and the factor four over one sample of it is the margin for the order.  It is never taken from
the GPU's output.  The loss keeps 1e-5 relative.

Every case prints, per parameter, the GPU's distance and the float32 oracle's distance as shares of the tolerance used.
Measured on an MI355X (one line per case; `pytest -s` prints every parameter):

  case                                         loss  worst gpu / tol                  fp32 oracle / tol  / project tol   4 x fp32 oracle is the tolerance of
  b512_d64_k8_m32                             0.005  0.001 entity_emb_matrix                      0.094          0.094   -
  b512_d64_k32_m32                            0.024  0.003 agg_0_0_weights                        0.095          0.095   -
  b1024_d32_k16_m64                           0.002  0.004 agg_0_0_weights                        0.250          0.395   relation_emb_KGE_matrix
  no_uo_b1024                                 0.005  0.002 agg_0_0_bias                           0.250          0.395   relation_emb_KGE_matrix
  ps_only_b1024                               0.007  0.001 entity_emb_matrix                      0.250          0.395   relation_emb_KGE_matrix
  ho_only_uo_kg_eh_b1024                      0.003  0.002 agg_0_0_weights                        0.250          0.395   relation_emb_KGE_matrix
  r136_b512_d64                               0.060  0.001 entity_emb_matrix                      0.010          0.010   -
  b4096_d64_k8_m32 (item grad separate)      0.072  0.003 agg_0_0_weights                        0.250          0.753   relation_emb_KGE_matrix
  b4096_d64_k8_m32 (item grad in kernel)     0.055  0.003 agg_0_0_weights                        0.250          0.753   relation_emb_KGE_matrix

  loss: |gpu - float64| as a share of 1e-5 relative.  "worst gpu / tol": the parameter where the GPU is closest to its
  tolerance.  "fp32 oracle": the float32 CPU oracle's distance from float64 for ITS worst parameter (always
  relation_emb_KGE_matrix), as a share of the tolerance used and of the project's 2e-4 * max|g| + 1e-7 alone.
  The GPU turns out far inside its tolerance (at most 0.004 of it), closer to float64 than the float32 CPU oracle is:
  on relation_emb_KGE_matrix, where the oracle's float32 chain through the materialised [B, Nm, D, D] lookup loses
  most, the GPU's distance rounds to 0.000.  The margin of four is therefore unused today; it stays as derived.
  Three applied steps at B 1 024 (tolerance per step: the larger of 1e-5 relative and 4 x the float32 CPU trajectory's
  distance from float64; the former was the larger at every step), shares of it at steps 1 / 2 / 3: eager 0.006 /
  0.005 / 0.004, graphed 0.006 / 0.007 / 0.006, float32 CPU trajectory 0.003 / 0.014 / 0.013.  Before Trainer.lr_t
  took the bias correction from the float32 betas the optimizer kernel works with, the GPU stood at 0.012 / 0.248 /
  0.563: every step was 6.4e-6 too long (decimal 0.999 on the host, float32(0.999) in the kernel), which this test found.
"""
import functools

import numpy as np
import pytest
import torch

from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from oracle import train_ref

pytestmark = pytest.mark.gpu

N_ENTITY, N_USER = 20011, 300

CASES = {
    # the four sizes at which the float32 oracle was measured against float64 (0.09 ... 0.75 of the tolerance)
    "b512_d64_k8_m32": dict(batch_size=512, dim=64, neighbor_sample_size=8, n_memory=32),
    "b512_d64_k32_m32": dict(batch_size=512, dim=64, neighbor_sample_size=32, n_memory=32),
    "b1024_d32_k16_m64": dict(batch_size=1024, dim=32, neighbor_sample_size=16, n_memory=64),
    "b4096_d64_k8_m32": dict(batch_size=4096, dim=64, neighbor_sample_size=8, n_memory=32),
    # other presets at B 1 024
    "no_uo_b1024": dict(batch_size=1024, dim=32, neighbor_sample_size=16, n_memory=64, ablation="no_uo"),
    "ps_only_b1024": dict(batch_size=1024, dim=32, neighbor_sample_size=16, n_memory=64, ablation="ps_only"),
    "ho_only_uo_kg_eh_b1024": dict(batch_size=1024, dim=32, neighbor_sample_size=16, n_memory=64,
                                   ablation="ho_only_uo_kg_eh"),
    # 136 relations at dim 64: the dV block of a (pair, hop) does not fit the key-addressing backward's LDS budget
    "r136_b512_d64": dict(batch_size=512, dim=64, neighbor_sample_size=8, n_memory=32, n_relation=136),
}


def make_case(name, seed=90):
    kw = dict(CASES[name])
    n_relation = kw.pop("n_relation", 12)
    kw.setdefault("ablation", "all")
    args = make_args(h_hop=2, n_mix_hop=1, p_hop=2, l2_weight=1e-3, l2_agg_weight=1e-4, lr=1e-2, **kw)
    case = synth.small_case(args, n_user=N_USER, n_entity=N_ENTITY, n_relation=n_relation, seed=seed, zero_rows=3)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=seed + 1, random_agg_bias=True)
    labels = (np.arange(args.batch_size) % 2).astype(np.float32)
    return args, case, params, labels


def cpu_feed(case, labels):
    return (case.adj_entity, case.adj_relation, case.users, case.items, labels, case.memories_h, case.memories_r,
            case.memories_t)


@functools.lru_cache(maxsize=2)
def oracles(name):
    """(float64 loss, float64 grads, float32-oracle grads) of a case; cached: two tests share the largest case."""
    args, case, params, labels = make_case(name)
    l64, g64, _, _ = train_ref.loss_and_grads(args, params, *cpu_feed(case, labels), dtype=torch.float64)
    _, g32, _, _ = train_ref.loss_and_grads(args, params, *cpu_feed(case, labels))
    return l64, g64, g32


def dev_feed(model, case, labels):
    dev = model.device
    up = lambda a: torch.from_numpy(a).to(dev)
    return (up(case.users), up(case.items), up(labels), [up(m) for m in case.memories_h],
            [up(m) for m in case.memories_r], [up(m) for m in case.memories_t])


def check_against_float64(what, got, loss, l64, g64, g32):
    assert abs(loss - l64) <= 1e-5 * abs(l64), (what, loss, l64)
    assert set(g32) == set(g64)
    worst = ("", 0.0, 0.0)
    failures = []
    print(f"\n{what}: loss {loss:.8f} vs float64 {l64:.8f} ({abs(loss - l64) / abs(l64) / 1e-5:.3f} of 1e-5 relative)")
    print(f"  {'parameter':<28}{'gpu / tol':>10}{'fp32 oracle / tol':>19}{'fp32 oracle / project tol':>27}   tolerance from")
    for name, g in g64.items():
        assert name in got, f"{what}: no gradient for {name}"
        project = 2e-4 * max(np.abs(g).max(), 1e-8) + 1e-7
        own = float(np.abs(g32[name].astype(np.float64) - g).max())
        tol = max(project, 4.0 * own)
        err = float(np.abs(got[name].astype(np.float64) - g).max())
        print(f"  {name:<28}{err / tol:>10.3f}{own / tol:>19.3f}{own / project:>27.3f}   "
              f"{'project' if tol == project else '4 x fp32 oracle'}")
        if err / tol > worst[1]:
            worst = (name, err / tol, own / tol)
        if not err <= tol:
            failures.append(f"{name}: max abs err {err:.3e} vs tolerance {tol:.3e}")
    print(f"  worst: {worst[0]} gpu {worst[1]:.3f}, fp32 oracle {worst[2]:.3f}")
    assert not failures, f"{what}: " + "; ".join(failures)
    for name, g in got.items():
        if name not in g64:
            assert not np.any(g), f"{what}: {name} has a gradient but the reference has none"


def run_case(name, item_grad_max_batch=None):
    from mvin_amd.model import MVIN
    from mvin_amd.training import Trainer
    from mvin_amd import ops
    args, case, params, labels = make_case(name)
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params,
                 device="cuda:0")
    tr = Trainer(model)
    # the key-addressing backward keeps dV of a (pair, hop) in LDS exactly where it can also add the item's share
    dv_in_lds = ops.key_addressing_bwd_adds_item_grad(args.p_hop, args.n_memory, args.dim, case.n_relation)
    if item_grad_max_batch is not None:
        assert dv_in_lds, "case bug: the kernel cannot take the item gradient at this shape; both runs would be one path"
        tr.item_grad_in_kernel_max_batch = item_grad_max_batch
    if name.startswith("r136"):
        assert not dv_in_lds, "case bug: 136 relations were meant to push dV out of LDS into global memory"
    loss = tr.step(*dev_feed(model, case, labels), apply=False)
    torch.cuda.synchronize()
    got = tr.grads_by_reference_name()
    del tr, model
    what = name if item_grad_max_batch is None else f"{name} item_grad_in_kernel_max_batch={item_grad_max_batch}"
    check_against_float64(what, got, loss, *oracles(name))


@pytest.mark.parametrize("name", [n for n in CASES if n != "b4096_d64_k8_m32"])
def test_loss_and_every_gradient_at_timed_sizes(name, hip_lib):
    run_case(name)


@pytest.mark.parametrize("max_batch", [0, 1 << 20])
def test_b4096_with_the_item_gradient_separate_and_in_the_kernel(max_batch, hip_lib):
    """Trainer.item_grad_in_kernel_max_batch on both sides of the batch: dE[item] of V = E[item] . R_KGE by a separate
    product + scatter-add (0) and inside the key-addressing backward (above the batch)."""
    run_case("b4096_d64_k8_m32", max_batch)


def test_three_applied_steps_eager_and_graphed_follow_the_float64_trajectory(hip_lib):
    """B 1 024, a different batch every step.  Losses against loss_and_grads(float64) + AdamRef(float64).  Tolerance
    per step, derived as the gradient tolerance is: the larger of the loss tolerance of a single step (1e-5 relative)
    and four times the distance of the float32 CPU trajectory (float32 oracle + float32 AdamRef, run here) from the
    float64 one at that step -- after an Adam step, entries whose gradient is round-off move by a whole lr in a
    direction the precision decides, for the float32 oracle as for the GPU.  Never from the GPU's output.  Graphed
    against eager at the 2e-5 of test_gpu_train.py."""
    from mvin_amd.model import MVIN
    from mvin_amd.training import GraphedTrainer, Trainer
    name = "b1024_d32_k16_m64"
    args, _, params, _ = make_case(name)
    B = args.batch_size
    big = make_args(**dict(vars(args), batch_size=3 * B))
    case = synth.small_case(big, n_user=N_USER, n_entity=N_ENTITY, n_relation=12, seed=95, zero_rows=3)
    labels = (np.random.default_rng(96).random(3 * B) < 0.5).astype(np.float32)
    mk = lambda: MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation,
                      params=params, device="cuda:0")
    model_e, model_g = mk(), mk()
    tr_e, tr_g = Trainer(model_e), Trainer(model_g)
    gt = GraphedTrainer(tr_g, B, ids_dtype=torch.from_numpy(case.users).dtype)
    # beta1, beta2 and epsilon as the optimizer kernel is handed them: float32 (mvin_l2_adam_multi takes floats, as
    # TF's ApplyAdam holds them in the variable's dtype).  float32(0.999) is 1.3e-5 relative away from 0.999 in
    # 1 - beta2, 6.4e-6 in every step's length: a property of the number format, which a float64 reference run on the
    # decimal 0.999 would report as a drift of the losses (2.4e-6 and 5.6e-6 relative at steps 2 and 3, measured)
    hyper = dict(beta1=float(np.float32(tr_e.b1)), beta2=float(np.float32(tr_e.b2)), eps=float(np.float32(tr_e.eps)))
    assert (tr_e.b1, tr_e.b2, tr_e.eps) == (0.9, 0.999, 1e-8)
    ref_p = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    opt = train_ref.AdamRef(ref_p, lr=args.lr, dtype=np.float64, **hyper)
    p32 = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
    opt32 = train_ref.AdamRef(p32, lr=args.lr, **hyper)
    le, lg, l64, l32 = [], [], [], []
    dev = model_e.device
    up = lambda a: torch.from_numpy(a).to(dev)
    for s in range(3):
        cut = lambda x: np.ascontiguousarray(x[s * B:(s + 1) * B])
        c_u, c_i, c_l = cut(case.users), cut(case.items), cut(labels)
        mh, mr, mt = [cut(x) for x in case.memories_h], [cut(x) for x in case.memories_r], [cut(x) for x in case.memories_t]
        feed = (up(c_u), up(c_i), up(c_l), [up(x) for x in mh], [up(x) for x in mr], [up(x) for x in mt])
        le.append(tr_e.step(*feed))
        lg.append(float(gt.step(*feed).item()))
        rl, rg, _, _ = train_ref.loss_and_grads(args, ref_p, case.adj_entity, case.adj_relation, c_u, c_i, c_l, mh, mr, mt,
                                                dtype=torch.float64)
        l64.append(rl)
        ref_p = opt.step(ref_p, rg)
        rl, rg, _, _ = train_ref.loss_and_grads(args, p32, case.adj_entity, case.adj_relation, c_u, c_i, c_l, mh, mr, mt)
        l32.append(rl)
        p32 = opt32.step(p32, rg)
    assert tr_e.t == tr_g.t == 3
    np.testing.assert_allclose(lg, le, rtol=2e-5, atol=1e-7)
    print(f"\nthree steps at B {B}:")
    failures = []
    for s in range(3):
        own = abs(l32[s] - l64[s])
        tol = max(1e-5 * abs(l64[s]), 4.0 * own)
        print(f"  step {s + 1}: float64 {l64[s]:.6f}  eager {abs(le[s] - l64[s]) / tol:.3f}  graphed {abs(lg[s] - l64[s]) / tol:.3f}"
              f"  fp32 oracle {own / tol:.3f} of the tolerance ({'1e-5 relative' if tol > 4.0 * own else '4 x fp32 oracle'})")
        for who, l in (("eager", le[s]), ("graphed", lg[s])):
            if not abs(l - l64[s]) <= tol:
                failures.append(f"step {s + 1} {who}: {l} vs float64 {l64[s]} (tolerance {tol:.3e})")
    assert not failures, "; ".join(failures)
