"""Cases of mvin_score_l2_folded_fwd at dim 64 for tests/test_gpu_fold_two_launch.py, and the process that runs them through the
two-launch A/B variant.

mvin_score_l2_folded_fwd reads MVIN_L2_FOLD_TWO once per process: with it set, dim 64 takes the pair kernel in its ``fold = 1`` output mode
(launch_gather_attn_l2_agg: out0 and Z2 go to scratch rows) followed by l2_tail_fold_kernel (mvin_tail.hip) instead of the ONE launch of
mvin_fused_agg.hip.  So

    MVIN_L2_FOLD_TWO=1 python tests/fold_two_worker.py OUT.pkl

runs the fold-D64K16 / K32 / K64 cases of tests/test_gpu_fold_f64.py through that module's own helpers (every batch size x attention, the
four item patterns, tables of 1 / 7 / 17 entities), one case of 32768 + 33 pairs (the only size at which a workgroup of
l2_tail_fold_kernel walks a second tile, so the only one at which its look-ahead loads run) and the id cases, all against float64 by the
rule of that module, and pickles {"fails": {form id: [...]}, "stats": ..., "ids": ..., "out": {case key: (item_emb, scores, sigmoid)}}.
The test module runs the same launches in its own process (the one-launch default) and compares the bits."""
import os
import pickle
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_fold_f64 as ff                               # noqa: E402
from fold_ref import fold_reference                          # noqa: E402

KS = (16, 32, 64)
BIG_K, BIG_B = 16, 32768 + 33                                # 1025 tiles of 32 pairs for the 1024 workgroups of l2_tail_fold_kernel
CHUNK = 4096                                                 # pairs per evaluation of the reference ([pairs, K, K, D] in float64)


def fid_of(K):
    """The key of the variant's figures (none of test_gpu_fold_f64.TAIL_BOUNDS_HOLD, which was measured on the one-launch form: the
    variant is held to the relative rule)."""
    return f"two-D64K{K}"


def cases(K):
    """(key, world, case, attention, biases) of the form fold-D64K<K>: the loops of test_every_batch_size_against_float64,
    test_item_patterns_against_float64 and test_tables_around_one_tile_of_rows."""
    for ai, att in enumerate(ff.ATTENTION):
        for bi, B in enumerate(ff.batch_sizes(K)):
            ax = ff._axes(bi, ai, att)
            w = ff._world(64, K, ff.N_ENTITY, ax["nR"], "counts")
            yield f"K{K} sizes att={att} B={B} {ax}", w, ff._case(w, ax["pattern"], B, ax["i64"], ax["uo_is_q"], seed=1000 * bi + ai), att, ax["bias"]
    for pattern in ff.PATTERNS:
        w = ff._world(64, K, ff.N_ENTITY, 7, "counts")
        for n, (B, att, i64, uo_is_q, bias) in enumerate(ff.pattern_cases(K)):
            yield (f"K{K} {pattern} B={B} att={att} i64={i64} uo_is_q={uo_is_q} bias={bias}", w,
                   ff._case(w, pattern, B, i64, uo_is_q, seed=77 + n, item_seed=n), att, bias)
    for n_entity in (1, 7, 17):
        for n, (B, att, nR, i64, bias) in enumerate(ff.small_table_cases(K)):
            w = ff._world(64, K, n_entity, nR, "random")
            yield (f"K{K} n_entity={n_entity} B={B} att={att} nR={nR}", w,
                   ff._case(w, "stride" if n % 2 == 0 else "runs", B, i64, n == 3, seed=300 + n), att, bias)


def big_case():
    w = ff._world(64, BIG_K, ff.N_ENTITY, 7, "counts")
    return f"K{BIG_K} second tile B={BIG_B}", w, ff._case(w, "stride", BIG_B, True, False, seed=4242), "unit", True


def launch(w, c, att, bias):
    """The case's launch on freshly built tables (run twice: equal bits) -> (item_emb, scores, sigmoid)."""
    t0, t1 = ff._logits(w, att)
    return ff._launch(w, "fold", ff._tables(w, "fold", t0, bias), c.items, t0, t1, c.q, c.uo, bias)


def chunked_references(w, c, att, bias):
    """ff._references with the reference evaluated over at most CHUNK pairs at a time."""
    t0, t1 = ff._logits(w, att)
    b0, b1, b2, a0, a1, bmix = w.bias if bias else (None,) * 6
    items, q, uo = c.ext
    r64, r32 = [], []
    for lo in range(0, items.shape[0], CHUNK):
        sl = slice(lo, lo + CHUNK)
        args = (w.E, w.ae, w.ar, items[sl], t0, t1, q[sl], uo[sl], w.W0, b0, w.W1, b1, w.W2, b2, w.A0, a0, w.A1, a1, w.Wmix, bmix, w.K)
        r64.append(fold_reference(*args)[2:])
        r32.append(fold_reference(*args, dtype=torch.float32)[2:])
    r64, r32 = ([torch.cat([r[i] for r in rs]) for i in range(3)] for rs in (r64, r32))
    yard = [float((b.double() - a).abs().max()) for a, b in zip(r64, r32)]
    return [r[: c.B] for r in r64], [r[: c.B] for r in r32], yard


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def main(path):
    res = {"fails": {}, "out": {}, "ids": {}, "cases": {}}
    for K in KS:
        fid = fid_of(K)
        fails = res["fails"].setdefault(fid, [])
        n = 0
        for key, w, c, att, bias in cases(K):
            keep = []
            try:
                ff._run_case(fid, w, "fold", c, att, bias, key, fails, keep=keep)
                res["out"][key] = host(keep[-1])
            except AssertionError as e:                          # (two runs of one launch differ, a world that is not what it claims)
                fails.append(f"{key}: {' '.join(str(e).split())[:300]}")
            n += 1
        res["cases"][fid] = n
        for i64 in (True, False):
            try:
                res["ids"][(fid, i64)] = ff.out_of_range_ids_check(("fold", 64, K), i64)
            except AssertionError as e:
                res["ids"][(fid, i64)] = [f"{' '.join(str(e).split())[:300]}"]
    key, w, c, att, bias = big_case()
    fails = res["fails"].setdefault("big", [])
    got = launch(w, c, att, bias)
    ff._compare(fid_of(BIG_K) + "@B=32801", key, got, chunked_references(w, c, att, bias), fails)
    res["out"][key] = host(got)
    res["stats"] = {k: list(v) for k, v in ff.STATS.items()}
    with open(path, "wb") as f:
        pickle.dump(res, f, protocol=4)


if __name__ == "__main__":
    assert os.environ.get("MVIN_L2_FOLD_TWO") == "1", "this process exists to run the folded form as pair kernel + l2_tail_fold_kernel"
    main(sys.argv[1])
