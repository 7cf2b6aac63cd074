"""The case list of tests/tail_worker.py without a device: every EXACT case is built and its float64 reference passes the case-bug checks
of ``exact()`` (sum of |terms| below 2^24 for every output, the reference an integer), the id rule of mvin_l2_tail_fwd as the worker
states it, and the shapes and options the GPU module claims."""
import numpy as np
import torch

import tail_worker as tw


def test_every_exact_case_fits_float32():
    worst = {}
    names = [n for n in tw.CASES if n.startswith("exact_")]
    assert len(names) >= 3 * len(tw.B_LIST)
    for name in names:
        case = tw.Case(name, tw.CASES[name])
        ref, mag = tw.reference(case), tw.magnitude(case)
        for nm, r, m in zip(("item_emb", "scores"), ref, mag):
            tw.exact(r.numpy(), r.numpy(), m.numpy(), 1, f"{name} {nm}")
            worst[(case.D, nm)] = max(worst.get((case.D, nm), 0.0), float(m.max()))
        relu_on = float((ref[0] != 0).double().mean())
        assert relu_on > 0.5, f"{name}: item embeddings mostly zero"
        assert case.spec["null"] in ("both", "sig") or float(ref[1].abs().max()) > 0
    print("worst sum of |terms|:", worst)
    assert worst[(64, "scores")] < 2.0 ** 24 / 8              # (measured 9.4e5: room for every evaluation order)


def test_bf16_tables_hold_bf16_values():
    for name, spec in tw.CASES.items():
        if spec.get("bf16"):
            case = tw.Case(name, spec)
            assert np.array_equal(tw.to_bf16(case.E), case.E)


def test_ids_are_clamped_whole_as_unsigned_64_bit_numbers():
    n = tw.N_ENTITY
    assert tw.clamp_tail_ids(np.array(tw.BAD_IDS64 + (0, 5, n - 1, n), dtype=np.int64), n).tolist() == [n - 1] * len(tw.BAD_IDS64) + [0, 5, n - 1, n - 1]
    assert tw.clamp_tail_ids(np.array(tw.BAD_IDS32 + (3,), dtype=np.int32), n).tolist() == [n - 1] * len(tw.BAD_IDS32) + [3]
    assert 2 ** 32 + 5 in tw.BAD_IDS64 and 5 < n - 1          # an id whose low word is a valid row: the two rules differ there
    for name in (k for k in tw.CASES if k.startswith("ids_")):
        case = tw.Case(name, tw.CASES[name])
        bad = tw.BAD_IDS64 if case.spec["i64"] else tw.BAD_IDS32
        assert sorted(set(int(v) for v in case.items[case.bad_at])) == sorted(bad)
        assert len({int(r) // 16 for r in case.bad_at}) >= 4 and int(case.bad_at.max()) < case.B      # several wave tiles


def test_shapes_and_options():
    for fam, Bs in (("exact", {D: tw.B_LIST for D in tw.DIMS}), ("real", {16: tw.B_SUBSET, 32: tw.B_SUBSET, 64: tw.B_LIST})):
        for D in tw.DIMS:
            specs = [dict(tw.DEFAULTS, **s) for n, s in tw.CASES.items() if n.startswith(fam + "_") and s["D"] == D]
            assert {s["B"] for s in specs} >= set(Bs[D])
            assert D != 64 or {s["B"] for s in specs if tw.flash_applies(s)} >= set(Bs[D])
    walks = {(s["D"], s["B"]) for n, s in tw.CASES.items() if n.endswith("_walk")}
    assert walks == {(64, 49152 + 213), (64, 32768 + 33), (32, 70000), (16, 70000)}
    assert all(dict(tw.DEFAULTS, **s)["i64"] for n, s in tw.CASES.items() if n.endswith("_walk"))
    real = tw.Case("real_probe", dict(D=16, B=3, real=True))
    assert real.n == tw.YARD_ROWS and real.q.shape == (256, 16) and abs(float(real.q.std()) - 0.3) < 0.02
    assert tw.reference(real)[0].shape == (256, 16) and tw.reference(real, torch.float32)[0].dtype == torch.float32
