"""-m gpu: the guard of the training step through Trainer / GraphedTrainer / harness.train (Trainer.set_guard:
mvin_grad_guard + mvin_l2_adam_multi_guarded between the backward and the update), on the small training case of
tests/test_gpu_train_ranked.py: dim 16, fan-out 4, 2 hops, batches of 40 to 64 rows.

Byte comparisons and float atomics.  The backward accumulates with float atomics, so two trainers that compute the SAME step
independently differ in the last bits of their gradients (the suite compares such twins at rtol 1e-5).  Where a test asks for
byte identity between two trainers, the second one therefore does not recompute the gradient: it is handed the flat gradient
buffer the first one's step produced (copied on the stream right before that trainer's own ``_apply_update``, also inside a
captured graph) and runs its own ``_apply_update`` on it -- the same launches ``enqueue`` ends in.  What is compared is then
exactly what the guard may or may not change: the update.  The independently recomputed twin is checked as well, at the
suite's twin tolerance.

Tolerances: parameters against the float64 oracle at the project's 2e-4 * max|ref| + 1e-7 per tensor; the norm against
sqrt(fsum(e^2)) at n * 2^-53 relative (tests/test_gpu_grad_guard.py derives it).
"""
import math

import numpy as np
import pytest
import torch

import grad_guard_oracle as go
from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

pytestmark = pytest.mark.gpu

B = 48


def build(seed=70, batch=B):
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, l2_weight=1e-3,
                     l2_agg_weight=1e-4, lr=1e-2, batch_size=batch)
    case = synth.small_case(args, n_user=12, n_entity=120, n_relation=5, seed=seed, zero_rows=3)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=seed + 1, random_agg_bias=True)
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params,
                 device="cuda:0")
    return args, case, params, model


def batches(model, case):
    """Three batches of the case on the device: A = its rows, B = a permutation of them with the labels flipped, P = A with
    labels[0] = nan (a poisoned batch: the cross-entropy's gradient of that row is NaN)."""
    dev = model.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    labels = (np.arange(B) % 2).astype(np.float32)
    perm = np.random.default_rng(3).permutation(B)

    def feed(rows, lab):
        return (t(case.users[rows]), t(case.items[rows]), t(lab), [t(m[rows]) for m in case.memories_h],
                [t(m[rows]) for m in case.memories_r], [t(m[rows]) for m in case.memories_t])
    poisoned = labels.copy()
    poisoned[0] = np.nan
    return feed(np.arange(B), labels), feed(np.arange(B), poisoned), feed(perm, 1.0 - labels[perm])


def snapshot(tr):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy().copy() for t in (tr._m, tr._v)) + \
        tuple(p.detach().cpu().numpy().copy() for p in tr.params.values())


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def spy_gradients(tr):
    """Record the flat gradient buffer as ``tr._apply_update`` finds it, on the stream (so a captured step records it on
    every replay); behaviour is unchanged."""
    snap = torch.zeros_like(tr._g)
    inner = tr._apply_update

    def spy(loss_acc, apply, lr_dev=None):
        if apply:
            snap.copy_(tr._g)
        return inner(loss_acc, apply, lr_dev)
    tr._apply_update = spy
    return snap


def update_from(tr, grad):
    """One applied step of ``tr`` on the recorded gradient buffer ``grad``: the tail of ``enqueue``."""
    tr._g.copy_(grad)
    tr._apply_update(torch.zeros(1, dtype=torch.float32, device=tr._g.device), True)
    tr.m.invalidate()


# =============================================================================================== 1. on but idle
@pytest.mark.parametrize("graphed", [False, True])
def test_an_idle_guard_changes_no_bit_of_the_update(graphed, hip_lib):
    from mvin_amd.training import GraphedTrainer, Trainer
    _, case, _, model_g = build()
    _, _, _, model_u = build()
    _, _, _, model_i = build()
    tr_g = Trainer(model_g, clip_norm=1e30, skip_nonfinite=True)
    tr_u, tr_i = Trainer(model_u), Trainer(model_i)
    assert tr_g.guard_on and not tr_u.guard_on and tr_u.guard_key() is None
    feeds = batches(model_g, case)
    grad = spy_gradients(tr_g)
    stepper = GraphedTrainer(tr_g, B, ids_dtype=feeds[0][0].dtype) if graphed else tr_g
    assert tr_g.guard_stats()["steps"] == 0                       # capture and its warm-up ran no guarded step
    exact_twins = True
    for feed in (feeds[0], feeds[2], feeds[0]):
        loss_g = stepper.step(*feed)
        loss_g = float(loss_g.item()) if graphed else loss_g
        update_from(tr_u, grad)                                   # unguarded, the same gradient buffer
        loss_i = tr_i.step(*feed)                                 # unguarded, recomputed independently
        assert same_bytes(snapshot(tr_g), snapshot(tr_u)), "a guard that neither clips nor skips changed the update"
        np.testing.assert_allclose(loss_g, loss_i, rtol=2e-5, atol=1e-7)
        exact_twins &= same_bytes(snapshot(tr_g), snapshot(tr_i))
    print(f"independently recomputed unguarded twin byte-identical after 3 steps: {exact_twins}")
    for a, b in zip(snapshot(tr_g), snapshot(tr_i)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6)
    st = tr_g.guard_stats()
    assert st["steps"] == st["applied"] == 3 == tr_g.t == tr_u.t and st["clipped_steps"] == st["skipped_steps"] == 0
    assert st["last_nonfinite"] == 0 and st["norm_max"] >= st["norm_mean"] > 0
    e = tr_g._g.detach().cpu().numpy()                            # last_grads: written back unscaled, L2 terms included
    exact = math.sqrt(go.sumsq(e))
    print(f"last_norm {st['last_norm']!r} vs {exact!r}")
    assert abs(st["last_norm"] - exact) <= e.size * 2.0 ** -53 * exact


# =============================================================================================== 2. clipping
def test_a_clipped_step_is_adam_on_the_scaled_gradient(hip_lib):
    from mvin_amd.training import Trainer
    args, case, params, model_u = build()
    _, _, _, model_g = build()
    feeds = batches(model_u, case)
    tr_u = Trainer(model_u)
    tr_u.step(*feeds[0])
    torch.cuda.synchronize()
    grads = {k: g.detach().cpu().numpy().astype(np.float64) for k, g in tr_u.last_grads.items()}
    norm = math.sqrt(go.sumsq(tr_u._g.detach().cpu().numpy()))
    c = np.float32(0.5 * norm)
    tr_g = Trainer(model_g, clip_norm=float(c))
    p0 = {k: v.astype(np.float64) for k, v in zip(tr_g.params, snapshot(tr_g)[2:])}
    tr_g.step(*feeds[0])
    st = tr_g.guard_stats()
    assert st["clipped_steps"] == 1 and st["applied"] == 1 and st["skipped_steps"] == 0
    assert abs(st["last_norm"] - norm) <= 1e-5 * norm              # twins: float atomics reorder the gradient's sums
    # the float64 oracle's step on grads * c / norm, from the start parameters under the trainer's names
    opt = go.GuardedAdam(p0, args.lr, float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8)))
    ref = opt.step(dict(p0), grads, scale=np.float32(float(c) / norm))
    got = dict(zip(tr_g.params, snapshot(tr_g)[2:]))
    for k, r in ref.items():
        tol = 2e-4 * np.abs(r).max() + 1e-7
        err = np.abs(got[k].astype(np.float64) - r).max()
        moved = np.abs(r - p0[k]).max()
        print(f"  {k}: {err / tol:.3f} of tolerance (largest update {moved:.3e})")
        assert err <= tol, f"{k}: max abs err {err:.3e} vs tolerance {tol:.3e}"
    per = tr_g.grad_norms()
    flat = [v for val in per.values() for v in (val if isinstance(val, list) else [val])]
    assert set(per) == set(tr_g.params) and isinstance(per["transfer_W"], list) and len(flat) == tr_g._nseg
    assert abs(math.sqrt(math.fsum(v * v for v in flat)) - st["last_norm"]) <= 1e-12 * st["last_norm"]
    # last_grads stay the unscaled gradients
    g_after = math.sqrt(go.sumsq(tr_g._g.detach().cpu().numpy()))
    assert abs(g_after - st["last_norm"]) <= tr_g._total * 2.0 ** -53 * g_after


# =============================================================================================== 3. a skipped step
@pytest.mark.parametrize("graphed", [False, True])
def test_a_skipped_step_never_happened(graphed, hip_lib):
    from mvin_amd.training import GraphedTrainer, Trainer
    _, case, _, model_1 = build()
    _, _, _, model_2 = build()
    tr_1 = Trainer(model_1, clip_norm=0.05, skip_nonfinite=True)       # clipping too: the small norm of this case is above it
    tr_2 = Trainer(model_2, clip_norm=0.05, skip_nonfinite=True)
    A, P, Bt = batches(model_1, case)
    grad = spy_gradients(tr_1)
    stepper = GraphedTrainer(tr_1, B, ids_dtype=A[0].dtype) if graphed else tr_1
    graph = stepper.graph if graphed else None
    read = (lambda x: float(x.item())) if graphed else (lambda x: x)
    assert math.isfinite(read(stepper.step(*A)))
    update_from(tr_2, grad)
    after_a = snapshot(tr_1)
    block_a = tr_1._guard_block().copy()
    assert math.isnan(read(stepper.step(*P)))                          # the poisoned batch's loss says so ...
    st = tr_1.guard_stats()
    assert st["skipped_steps"] == 1 and st["applied"] == 1 and st["steps"] == 2 and st["last_nonfinite"] > 0
    assert same_bytes(snapshot(tr_1), after_a), "a skipped step wrote a parameter or a moment"      # ... and nothing moved
    block_p = tr_1._guard_block()
    assert block_p["lr_t"].tobytes() == block_a["lr_t"].tobytes() and block_p["ok"] == 0
    assert math.isfinite(read(stepper.step(*Bt)))
    update_from(tr_2, grad)
    assert same_bytes(snapshot(tr_1), snapshot(tr_2)), "A, P, B did not end where A, B ends"
    s1, s2 = tr_1.guard_stats(), tr_2.guard_stats()
    assert (s1["skipped_steps"], s1["applied"], s1["steps"], tr_1.t) == (1, 2, 3, 3)
    assert (s2["skipped_steps"], s2["applied"], s2["steps"], tr_2.t) == (0, 2, 2, 2)
    assert s1["clipped_steps"] == s2["clipped_steps"] == 2
    assert tr_1._guard_block()["lr_t"] == np.float32(tr_1.lr_t(2))      # the second APPLIED step's size, not the third's
    if graphed:
        assert stepper.graph is graph and stepper.guard == tr_1.guard_key()          # three replays of one capture


# =============================================================================================== 4. recapture
N_USER, N_ENTITY, N_REL, N_ITEM = 12, 200, 5, 40


def harness_case(seed=3):
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=40, lr=1e-2)
    rng = np.random.default_rng(seed)
    adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 4, seed=seed + 1)
    uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=seed + 2)
    params = init_params(args, N_USER, N_ENTITY, N_REL, seed=seed + 3, random_agg_bias=True)
    model = MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, params=params, device="cuda:0")
    d = np.stack([rng.integers(0, N_USER, 400), rng.integers(0, N_ITEM, 400), rng.integers(0, 2, 400)], axis=1)
    _, first = np.unique(d[:, :2], axis=0, return_index=True)
    data = d[np.sort(first)].astype(np.int64)
    n = data.shape[0]
    return args, model, uts, (data[:n * 6 // 10], data[n * 6 // 10:n * 8 // 10], data[n * 8 // 10:])


def test_switching_the_guard_recaptures_changing_its_values_does_not(hip_lib):
    from mvin_amd import harness
    from mvin_amd.training import Trainer
    args, model, uts, (train, _, _) = harness_case()
    feeder = harness.DeviceFeeder(model, uts)
    model.trainer = Trainer(model)
    run = lambda: harness.train_epoch_device(feeder, train.copy(), args.batch_size, rng=np.random.default_rng(1), graph=True)
    run()
    g_off = model._graphed_trainer
    assert g_off is not None and g_off.guard is None
    model.trainer.set_guard(clip_norm=1.0)
    with pytest.raises(RuntimeError, match="guard"):
        g_off.replay()                                                  # a stale graph refuses; the harness builds a new one
    losses = run()
    g_on = model._graphed_trainer
    assert g_on is not g_off and g_on.guard == model.trainer.guard_key() is not None
    steps = model.trainer.guard_stats()["steps"]
    assert steps == len(losses) > 0
    model.trainer.set_guard(clip_norm=1e-3, skip_nonfinite=True)        # other values, same launches
    run()
    assert model._graphed_trainer is g_on
    st = model.trainer.guard_stats()
    assert st["steps"] == 2 * steps and st["clipped_steps"] >= steps    # ... and the new clip is the one in force
    model.trainer.set_guard()                                           # off again
    assert model.trainer.t == st["applied"]                             # the unguarded steps go on from the applied ones
    run()
    assert model._graphed_trainer is not g_on and model._graphed_trainer.guard is None
    assert model.trainer.guard_stats()["steps"] == 2 * steps            # no guarded step since


# =============================================================================================== 5. harness.train
def test_train_reports_the_guard_in_the_epoch_record(hip_lib):
    from mvin_amd import harness
    args, model, uts, split = harness_case()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 1, 2, 5, False
    full = (N_USER, N_ITEM, N_ENTITY, N_REL) + split + (None, None, uts)
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), objective="bpr", negatives="hard",
                            n_neg=2, pool=6, clip_norm=1e-3)
    rec = hist[0]
    assert {"grad_norm", "clipped_steps", "skipped_steps"} <= set(rec)
    assert rec["grad_norm"]["max"] >= rec["grad_norm"]["mean"] > 0
    assert rec["clipped_steps"] >= 1 and rec["skipped_steps"] == 0 and np.isfinite(rec["loss"])
    assert model.trainer.guard_on and model.trainer.clip_norm == 1e-3
    # a second guarded epoch counts from zero again
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), objective="bpr", negatives="hard",
                            n_neg=2, pool=6, clip_norm=1e-3, skip_nonfinite=True)
    assert hist[0]["clipped_steps"] == rec["clipped_steps"]
    # guard off: the record of before, and the trainer's guard is off
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), objective="bpr", negatives="hard",
                            n_neg=2, pool=6)
    assert not {"grad_norm", "clipped_steps", "skipped_steps"} & set(hist[0])
    assert set(hist[0]) == {"epoch", "loss", "pairwise_acc", "hard_rate", "pool_rate", "train", "eval", "test"}
    assert not model.trainer.guard_on
