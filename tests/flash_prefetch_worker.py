"""Cases of tests/test_gpu_flash_prefetch.py and the process that runs them under another setting of the flash kernel's switches.

MVIN_KAF_PREFETCH and MVIN_KAF_GRID are read once per process by the launcher (mvin_keyaddr_flash.hip), so the forms that are
compared bit for bit each run in a process of their own:

    MVIN_KAF_PREFETCH=0 python tests/flash_prefetch_worker.py OUT.pt

runs every case below and saves {case name: user_o or scores} (CPU tensors)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, N_ENTITY = 64, 5000
CANARY_I32, CANARY_F32, N_CANARY = 0x5A5A5A5A, 12345.0, 64

SHAPES = [(1, 64, 9), (2, 64, 9), (2, 40, 9), (2, 33, 70), (3, 32, 9), (8, 8, 5), (2, 1, 1)]     # (P, Nm, nR)
BOUNDARY_COUNTS = [1, 16, 17, 32, 33, 64, 65, 128, 129]


def _kernel_cases():
    """name -> (P, Nm, nR, with h-set, item dtype, n_user, users kind, B)."""
    c = {}
    # slot boundaries (a slot is up to 64 pairs = two tiles of 32 = four column tiles of 16)
    c["counts_1_to_129"] = (2, 64, 9, True, torch.int64, 12, "counts", sum(BOUNDARY_COUNTS))
    c["one_user_600_pairs"] = (2, 64, 9, True, torch.int64, 5, "one", 600)               # ten slots of one segment
    # 40 of 3 000 users present: 3 055 slots of which ~95 are live, single holes between them and ~2 900 behind them
    # (at MVIN_KAF_GRID=1 a look-ahead round covers 256 slots: many rounds without a live one); the table ENDS in holes
    c["most_users_absent"] = (2, 64, 9, True, torch.int64, 3000, "few", 3500)
    c["one_pair"] = (2, 64, 9, True, torch.int64, 7, "random", 1)
    # the slot table's last word is a hole by construction (B / 64 + segments + 1 slots); here every slot before it is live
    c["last_slots_live"] = (2, 64, 9, True, torch.int64, 1, "one", 70)
    # who walks what: 494 slots, every wave of a one-workgroup grid crosses ~100 slot boundaries with a live prefetch
    c["many_slots"] = (2, 64, 9, True, torch.int64, 400, "random", 6000)
    for P, Nm, nR in SHAPES:
        for has_set in (True, False):
            for idt in (torch.int64, torch.int32):
                c["P%dNm%dnR%d_%s_%s" % (P, Nm, nR, "set" if has_set else "noset", "i64" if idt == torch.int64 else "i32")] = (
                    P, Nm, nR, has_set, idt, 300, "random", 1500)
    return c


KERNEL_CASES = _kernel_cases()
FORWARD_CASES = {"forward_users_B3500_u3000": (3500, 3000), "forward_users_B9000_u2000": (9000, 2000)}     # name -> (pairs, users)


def make_inputs(name):
    """Deterministic inputs of a kernel case (the same in every process)."""
    from mvin_amd import synth
    P, Nm, nR, has_set, idt, n_user, kind, B = KERNEL_CASES[name]
    seed = sorted(KERNEL_CASES).index(name)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7000 + seed)
    rnd = lambda *s: torch.rand(s, device=dev, generator=g) - 0.5     # noqa: E731
    E, R = rnd(N_ENTITY, D), rnd(nR, D, D) * 0.5
    w = rnd(D) if has_set else None
    n_o = P + (1 if has_set else 0)
    W, b = rnd(n_o * D, D) * 0.3, rnd(D)
    uts = torch.from_numpy(synth.ripple_sets(n_user, N_ENTITY, nR, P, Nm, seed=seed)).to(dev)
    if kind == "counts":
        ids = torch.randperm(n_user, device=dev, generator=g)[:len(BOUNDARY_COUNTS)]
        users = torch.repeat_interleave(ids, torch.tensor(BOUNDARY_COUNTS, device=dev))
        users = users[torch.randperm(B, device=dev, generator=g)]
    elif kind == "one":
        users = torch.full((B,), n_user // 2, device=dev, dtype=torch.int64)
    elif kind == "few":
        present = torch.randperm(n_user, device=dev, generator=g)[:40]
        users = present[torch.randint(0, 40, (B,), device=dev, generator=g)]
    else:
        users = torch.randint(0, n_user, (B,), device=dev, generator=g)
    assert users.shape == (B,)
    items = torch.randint(0, N_ENTITY, (B,), device=dev, generator=g).to(idt)
    return dict(P=P, Nm=Nm, nR=nR, has_set=has_set, n_user=n_user, B=B, E=E, R=R, w=w, W=W, b=b, uts=uts, users=users, items=items)


def run_kernel_case(name):
    """Two launches over a NaN-filled output with canaries behind the output and behind the scheduling scratch."""
    from mvin_amd import _lib, ops
    x = make_inputs(name)
    P, Nm, nR, has_set, n_user, B = x["P"], x["Nm"], x["nR"], x["has_set"], x["n_user"], x["B"]
    dev = x["E"].device
    assert ops.key_addressing_flash_supported(D, P, Nm, nR, N_ENTITY)
    rec = ops.build_user_records(x["uts"], P, nR, N_ENTITY)
    groups = ops.group_pairs_by_user(x["users"], n_user=n_user)
    tabs = ops.key_addressing_flash_prepare(x["E"], x["R"], x["w"], x["W"], P)
    n_ws = _lib.load().mvin_key_addressing_flash_ws_elems(B, n_user)
    first = None
    for _ in range(2):
        ws = torch.full((n_ws + N_CANARY,), CANARY_I32, dtype=torch.int32, device=dev)
        buf = torch.full((B + N_CANARY, D), CANARY_F32, device=dev)
        buf[:B] = float("nan")
        ops.key_addressing_flash(x["E"], tabs, rec, groups, x["items"], P, Nm, nR, has_set, x["b"], n_user, sched_ws=ws, out=buf[:B])
        torch.cuda.synchronize()
        assert torch.isfinite(buf[:B]).all(), f"{name}: a pair's row was not written"
        assert (buf[B:] == CANARY_F32).all(), f"{name}: write behind user_o"
        assert (ws[n_ws:] == CANARY_I32).all(), f"{name}: write behind the scheduling scratch"
        if first is None:
            first = buf[:B].clone()
        assert torch.equal(first, buf[:B]), f"{name}: two launches differ"
    return first


def run_forward_case(name):
    """MVIN.forward_users over the grouped users feed with the flash form of key addressing (one native call) -> scores."""
    from mvin_amd import synth
    from mvin_amd.config import make_args
    from mvin_amd.model import MVIN
    from mvin_amd.params import init_params
    B, n_user = FORWARD_CASES[name]
    K, H, P, Nm, nR, n_entity = 4, 2, 2, 64, 9, 500
    args = make_args(dim=D, neighbor_sample_size=K, h_hop=H, n_mix_hop=1, p_hop=P, n_memory=Nm, batch_size=B, ablation="all")
    rng = np.random.default_rng(B)
    adj_e, adj_r = synth.uniform_adjacency(n_entity, nR, K, seed=3)
    uts = synth.ripple_sets(n_user, n_entity, nR, P, Nm, seed=4)
    users = rng.integers(0, n_user, B, dtype=np.int64)
    items = rng.integers(0, n_entity, B, dtype=np.int64)
    params = init_params(args, n_user, n_entity, nR, seed=5, random_agg_bias=True)
    model = MVIN(args, n_user, n_entity, nR, adj_e, adj_r, params=params, device="cuda:0")
    model.group_min_pairs_per_user = 0
    model.small_max_batch = 0
    model.ka_flash = True
    dev = model.device
    out = model.forward_users(torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev), torch.from_numpy(uts).to(dev))
    torch.cuda.synchronize()
    assert any(t is not None for t in model._ka_flash_ws.values()), "the flash form of key addressing was expected"
    return out.scores.clone()


PINNED_ENV = {"MVIN_SMALL": "0", "MVIN_PRJ": "0"}            # the forms tests/conftest.py pins for the kernel test modules


def run_all():
    """Every case -> {name: CPU tensor}, under PINNED_ENV."""
    saved = {k: os.environ.get(k) for k in PINNED_ENV}
    os.environ.update(PINNED_ENV)
    try:
        out = {name: run_kernel_case(name).cpu() for name in KERNEL_CASES}
        out.update({name: run_forward_case(name).cpu() for name in FORWARD_CASES})
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


if __name__ == "__main__":
    torch.save(run_all(), sys.argv[1])
