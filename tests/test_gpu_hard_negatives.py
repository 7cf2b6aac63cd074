"""-m gpu: mvin_select_negatives (ops.select_negatives) bit for bit against the rule of tests/hard_neg_oracle.py: items, valid,
score bits and the four counts, over every sub-wave width of the kernel (Gp 2 .. 64), launches of one workgroup and of many,
heavy ties, masks, launch-shape independence, and against the selection kernel mvin_topk_rows whose comparator it shares."""
import numpy as np
import pytest
import torch

import hard_neg_oracle as ho

pytestmark = pytest.mark.gpu

GPS = [2, 3, 16, 17, 32, 33, 64]
N_GROUPS = [0, 1, 5, 257, 4099]
SEED, ROUND = 0xF123456789ABCDEF, (1 << 63) + 12345          # 64-bit on purpose
# five integers, both zeros, both infinities, NaNs of both signs with a payload
SPECIAL_BITS = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000], dtype=np.uint32)
TIE_POOL = np.concatenate([np.array([-2, -1, 0, 1, 2], dtype=np.float32), SPECIAL_BITS.view(np.float32)])


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def make_case(Gp, n, seed, masks=True):
    rng = np.random.default_rng(seed)
    scores = TIE_POOL[rng.integers(0, TIE_POOL.size, (n, Gp))]
    items = rng.integers(0, 1 << 40, (n, Gp)).astype(np.int64)
    key = rng.integers(-(1 << 63), (1 << 63) - 1, n).astype(np.int64)
    valid = None
    if masks:
        valid = (rng.random((n, Gp)) < 0.7).astype(np.float32)
        valid[::7, 1:] = 0.0                                   # fully masked groups
        valid[3::7, 1:] = 2.5                                  # any non-zero flag is "valid"
        valid[:, 0] = rng.integers(0, 2, n)                    # the flag of slot 0 is ignored
    return scores, items, valid, key


def modes(Gp):
    out = []
    for n_neg in sorted({n for n in (1, 2, Gp - 1) if 1 <= n <= Gp - 1}):
        for shortlist in sorted({s for s in (n_neg, (n_neg + Gp - 1) // 2, Gp - 1) if n_neg <= s <= Gp - 1}):
            out.append((n_neg, shortlist))
    return out


def launch(scores, items, valid, key, n_neg, shortlist, counts=None):
    from mvin_amd import ops
    out = ops.select_negatives(dev(scores), dev(items), dev(valid), n_neg, shortlist, SEED, ROUND, group_key=dev(key),
                               counts=counts, out_scores=True)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)


def check(got, want, what):
    for name, g, w in zip(("items", "valid", "score bits"), got, want[:3]):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differ in {bad.size} groups, first {bad[0]}: {g[bad[0]]} vs {w[bad[0]]}"


@pytest.mark.parametrize("Gp", GPS)
def test_kernel_equals_oracle(Gp, hip_lib):
    """Every (n_neg, shortlist) mode of this Gp, every launch size; the smaller launches are prefixes of the largest one's
    groups, so the oracle runs once per mode (a row does not depend on n_groups -- which is also what this checks)."""
    scores, items, valid, key = make_case(Gp, max(N_GROUPS), Gp)
    for n_neg, shortlist in modes(Gp):
        want = ho.select_negatives(scores, items, valid, n_neg, shortlist, SEED, ROUND, key)
        for n in N_GROUPS:
            counts = torch.zeros(4, dtype=torch.int64, device="cuda:0")
            got = launch(scores[:n], items[:n], valid[:n], key[:n], n_neg, shortlist, counts)
            what = f"Gp={Gp} n_neg={n_neg} shortlist={shortlist} n_groups={n}"
            check(got, [w[:n] for w in want[:3]], what)
            want_counts = want[3] if n == max(N_GROUPS) else \
                ho.select_negatives(scores[:n], items[:n], valid[:n], n_neg, shortlist, SEED, ROUND, key[:n])[3] if n else (0,) * 4
            assert tuple(counts.cpu().tolist()) == want_counts, what
            # containment: no output id from outside its own group
            assert (got[0][:, :, None] == items[:n, None, :]).any(axis=2).all(), what


@pytest.mark.parametrize("Gp", GPS)
def test_without_masks_keys_counts_or_scores_out(Gp, hip_lib):
    from mvin_amd import ops
    scores, items, _, _ = make_case(Gp, 257, 100 + Gp, masks=False)
    n_neg = min(2, Gp - 1)
    shortlist = (n_neg + Gp - 1) // 2
    want = ho.select_negatives(scores, items, None, n_neg, shortlist, 3, 1)
    got = ops.select_negatives(dev(scores), dev(items), None, n_neg, shortlist, 3, 1)
    assert len(got) == 2
    check([g.cpu().numpy() for g in got], want[:2], f"Gp={Gp}")


@pytest.mark.parametrize("Gp,n_neg,shortlist", [(8, 2, 5), (17, 4, 9), (64, 8, 20), (33, 32, 32)])
def test_a_row_depends_on_its_own_group_only(Gp, n_neg, shortlist, hip_lib):
    """The same groups shuffled, with their keys carried along, and a third of them in a launch of another size."""
    n = 1000
    scores, items, valid, key = make_case(Gp, n, 7 * Gp)
    base = launch(scores, items, valid, key, n_neg, shortlist)
    perm = np.random.default_rng(1).permutation(n)
    shuffled = launch(scores[perm], items[perm], valid[perm], key[perm], n_neg, shortlist)
    check(shuffled, [b[perm] for b in base], "shuffled")
    sub = perm[:333]
    part = launch(scores[sub], items[sub], valid[sub], key[sub], n_neg, shortlist)
    check(part, [b[sub] for b in base], "a smaller launch")
    again = launch(scores, items, valid, key, n_neg, shortlist)
    check(again, base, "the same launch twice")


def test_counts_accumulate_exactly_across_calls(hip_lib):
    a = make_case(17, 4099, 1)
    b = make_case(33, 300, 2)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    counts[2] = 1 << 40                                         # 64-bit sums
    launch(*a, 4, 8, counts)
    launch(*b, 2, 2, counts)
    wa = ho.select_negatives(a[0], a[1], a[2], 4, 8, SEED, ROUND, a[3])[3]
    wb = ho.select_negatives(b[0], b[1], b[2], 2, 2, SEED, ROUND, b[3])[3]
    want = [x + y for x, y in zip(wa, wb)]
    want[2] += 1 << 40
    assert counts.cpu().tolist() == want and wa[1] > 0 and wb[0] > 0


@pytest.mark.parametrize("Gp,n_neg", [(2, 1), (17, 4), (33, 32), (64, 10)])
def test_hardest_mode_agrees_with_topk_rows(Gp, n_neg, hip_lib):
    """shortlist == n_neg without masks: the chosen slots are mvin_topk_rows over scores[:, 1:] with k = n_neg -- one
    comparator (csrc/mvin_score_image.h), ties by position, NaN below -inf, in both kernels."""
    from mvin_amd import ops
    scores, _, _, _ = make_case(Gp, 513, 50 + Gp, masks=False)
    items = np.broadcast_to(np.arange(Gp, dtype=np.int64), scores.shape).copy()          # an item's id is its slot
    s = dev(scores)
    got = ops.select_negatives(s, dev(items), None, n_neg, n_neg, 1, 0)[0]
    ids, _ = ops.topk_rows(s[:, 1:], n_neg)
    assert torch.equal(got[:, 1:], ids.long() + 1) and bool((got[:, 0] == 0).all())
