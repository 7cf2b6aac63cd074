"""CPU: the negative-sampling rule of mvin_sample_negatives (tests/neg_oracle.py restates it), its uniformity and draw cap as
fixed computations, the C ABI's argument validation (nothing launched), the host plumbing of mvin_amd.data_prep
(interaction_csr, NegativeSampler with the kernel call replaced by the oracle) and the generated ISA of the kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import neg_oracle as no

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")
MAX_ITEMS = 1 << 20


def csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([x for r in rows for x in r], dtype=np.int32)
    return ptr, ids


# --------------------------------------------------------------------------- the rule
def test_rule_outputs_are_distinct_in_range_and_eligible():
    rng = np.random.default_rng(0)
    n_item = 200
    rows = [rng.integers(0, n_item, size=int(rng.integers(0, 120))).tolist() for _ in range(60)]
    counts = rng.integers(0, 90, size=60)
    ptr, ids = csr(rows)
    out_ptr, items, status = no.sample_negatives_scalar(ptr, ids, counts, n_item, seed=5, round=3)
    assert out_ptr.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    short = 0
    for u, row in enumerate(rows):
        got = items[out_ptr[u]:out_ptr[u + 1]].tolist()
        c = n_item - len(set(row))
        real = [x for x in got if x >= 0]
        assert len(real) == min(int(counts[u]), c)                    # exactly min(m, c)
        assert got[len(real):] == [-1] * (len(got) - len(real))       # padding only behind them
        assert len(set(real)) == len(real) and all(0 <= x < n_item for x in real)
        assert not set(real) & set(row)
        short += len(real) < len(got)
    assert status.tolist() == [short, int((items < 0).sum())]


def test_rule_m_equal_c_returns_every_eligible_item():
    n_item = 40
    row = [3, 17]
    got, draws = no.user_negatives_scalar(row, 38, n_item, 1, 0, 0)
    assert sorted(got) == sorted(set(range(n_item)) - set(row))
    assert draws <= no.draw_cap(n_item)


def test_rule_m_above_c_leaves_minus_one_and_counts_one_short_user():
    n_item = 10
    ptr, ids = csr([[0, 1, 2, 3, 4, 5, 6], []])
    out_ptr, items, status = no.sample_negatives_scalar(ptr, ids, [5, 4], n_item)
    first = items[:5].tolist()
    assert sorted(first[:3]) == [7, 8, 9] and first[3:] == [-1, -1]
    assert (items[5:] >= 0).all()
    assert status.tolist() == [1, 2]


def test_rule_ignores_out_of_range_and_repeated_exclusions():
    n_item = 50
    clean = [4, 9, 30]
    noisy = [30, -1, 4, 50, 9, 4, 4, 1000, -7, 30]
    a = no.user_negatives_scalar(clean, 47, n_item, 11, 2, 6)[0]
    b = no.user_negatives_scalar(noisy, 47, n_item, 11, 2, 6)[0]
    assert a == b and -1 not in a                                     # c = 47 either way: every slot filled


def test_rule_depends_on_seed_round_and_user_and_is_repeatable():
    n_item, m = 1000, 20
    base = no.user_negatives_scalar([], m, n_item, 1, 0, 0)[0]
    assert base == no.user_negatives_scalar([], m, n_item, 1, 0, 0)[0]
    assert base != no.user_negatives_scalar([], m, n_item, 2, 0, 0)[0]
    assert base != no.user_negatives_scalar([], m, n_item, 1, 1, 0)[0]
    assert base != no.user_negatives_scalar([], m, n_item, 1, 0, 1)[0]
    assert base != no.user_negatives_scalar([], m, n_item, 1 + (1 << 40), 0, 0)[0]     # the high seed bits count


def test_scalar_and_numpy_oracles_agree():
    rng = np.random.default_rng(1)
    for n_item in (1, 2, 7, 8, 33, 64, 65, 300, 5000):
        rows = [rng.integers(-3, n_item + 3, size=int(rng.integers(0, 2 * n_item))).tolist() for _ in range(12)]
        rows[0] = []
        counts = rng.integers(0, n_item + 3, size=12)
        counts[1] = 0
        ptr, ids = csr(rows)
        for seed, rnd in ((1, 0), ((1 << 33) + 5, 17)):
            a = no.sample_negatives_scalar(ptr, ids, counts, n_item, seed, rnd)
            b = no.sample_negatives_np(ptr, ids, counts, n_item, seed, rnd)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (n_item, seed, rnd)
    a = no.sample_negatives_scalar(None, None, [5, 0, 9], 12, 3, 1)
    b = no.sample_negatives_np(None, None, [5, 0, 9], 12, 3, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_numpy_draws_are_rnd_below():
    from oracle.prep_ref import rnd_below
    for n_item, seed, rnd, u in ((48091, 1, 0, 0), (1 << 20, (1 << 63) + 12345, (1 << 64) - 1, 23552), (3, 7, 9, 11)):
        x = no.draws_np(n_item, seed, rnd, u, 5, 70).tolist()
        assert x == [rnd_below(n_item, seed, 4, u, rnd, j) for j in range(5, 70)]


# --------------------------------------------------------------------------- uniformity and the cap (seeded: pass or fail)
@pytest.mark.parametrize("seed", [1, 2, 3, 7])
def test_rule_is_uniform_over_the_eligible_items(seed):
    """n_item = 64, exclusion = the 16 even ids below 32, m = 8, 20 000 users: Pearson's chi-square over the 48 eligible items
    against the uniform expectation, of how often each item is drawn and of how often it is drawn FIRST, stays below 109 --
    the 1 - 1e-6 quantile of chi-square with 47 degrees of freedom (Wilson-Hilferty).  Its expectation is 47."""
    n_item, m, n_user = 64, 8, 20000
    row = list(range(0, 32, 2))
    eligible = sorted(set(range(n_item)) - set(row))
    assert len(eligible) == 48
    counts = np.zeros(n_item, dtype=np.int64)
    firsts = np.zeros(n_item, dtype=np.int64)
    for u in range(n_user):
        got = no.user_negatives_scalar(row, m, n_item, seed, 0, u)[0]
        counts[got] += 1
        firsts[got[0]] += 1
    assert counts[row].sum() == 0 and counts.sum() == n_user * m
    for name, obs, total in (("counts", counts, n_user * m), ("first draws", firsts, n_user)):
        exp = total / 48.0
        chi2 = float((((obs[eligible] - exp) ** 2) / exp).sum())
        print(f"seed {seed}: chi-square of the {name} = {chi2:.1f}")
        assert chi2 < 109.0, (name, chi2)


def test_draw_cap_is_far_from_a_valid_request():
    """Taking all 38 eligible of 40 items for 5 000 users never comes near the 64 * n_item = 2 560 draw cap."""
    worst = 0
    for u in range(5000):
        got, draws = no.user_negatives_scalar([0, 39], 38, 40, 1, 0, u)
        assert -1 not in got
        worst = max(worst, draws)
    print(f"worst case: {worst} draws of {no.draw_cap(40)}")
    assert worst <= no.draw_cap(40)


# --------------------------------------------------------------------------- the C ABI (nothing is launched)
def header_functions():
    src = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(mvin_[a-z0-9_]+)\s*\(", src))


def test_symbols_declared_exported_and_bound(hip_lib):
    from mvin_amd import _lib
    for name in ("mvin_sample_negatives", "mvin_sample_negatives_supported"):
        assert name in header_functions()
        assert hasattr(hip_lib, name)
        assert name in _lib.SIGNATURES
    assert hip_lib.mvin_abi_version() == 12
    assert "#define MVIN_NEG_MAX_ITEMS (1 << 20)" in open(os.path.join(ROOT, "include", "mvin_hip.h")).read()


def test_supported_range(hip_lib):
    assert hip_lib.mvin_sample_negatives_supported(1) == 1
    assert hip_lib.mvin_sample_negatives_supported(MAX_ITEMS) == 1
    assert hip_lib.mvin_sample_negatives_supported(0) == 0
    assert hip_lib.mvin_sample_negatives_supported(MAX_ITEMS + 1) == 0
    assert hip_lib.mvin_sample_negatives_supported(-5) == 0


def test_argument_errors_return_codes_and_launch_nothing(hip_lib):
    """Null or dummy pointers only: a call that got past validation would fault on them."""
    one = C.c_void_p(16)
    f = hip_lib.mvin_sample_negatives

    def err(*args):
        rc = f(*args)
        msg = hip_lib.mvin_last_error()
        assert rc < 0 and b"mvin_sample_negatives" in msg, (rc, msg)
        return rc, msg

    # every required pointer
    for hole in range(4):
        ptrs = [one, one, one, one]                                   # counts, out_ptr, out_items, status
        ptrs[hole] = None
        rc, msg = err(one, one, ptrs[0], ptrs[1], 4, 100, 1, 0, ptrs[2], ptrs[3], None)
        assert rc == -1 and b"null" in msg
    # one of excl_ptr / excl_ids without the other
    assert err(one, None, one, one, 4, 100, 1, 0, one, one, None)[0] == -1
    assert err(None, one, one, one, 4, 100, 1, 0, one, one, None)[0] == -1
    # sizes
    rc, msg = err(None, None, one, one, -1, 100, 1, 0, one, one, None)
    assert rc == -2 and b"n_user=-1" in msg
    for bad in (0, -3, MAX_ITEMS + 1):
        rc, msg = err(None, None, one, one, 4, bad, 1, 0, one, one, None)
        assert rc == -3 and b"unsupported n_item" in msg
    from mvin_amd import _lib
    with pytest.raises(_lib.MvinHipError, match="unsupported n_item"):
        _lib.check(rc, "mvin_sample_negatives")


# --------------------------------------------------------------------------- host plumbing (torch on the CPU device)
def dict_of_sets(arrays, labels):
    rec = {}
    for a in arrays:
        for u, i, lab in np.asarray(a).tolist():
            if labels is None or lab == labels:
                rec.setdefault(u, set()).add(i)
    return rec


def splits(seed=0, n_user=30, n_item=25, n=400):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        d = np.stack([rng.integers(0, n_user - 3, size=n), rng.integers(0, n_item, size=n), rng.integers(0, 2, size=n)], axis=1)
        out.append(d.astype(np.int64))                                # users n_user-3 .. n_user-1 have no rows at all
    return out


@pytest.mark.parametrize("labels", [1, None])
def test_interaction_csr_matches_dict_of_sets(labels):
    from mvin_amd import data_prep
    n_user = 30
    arrays = splits()
    ptr, ids = data_prep.interaction_csr(arrays, n_user, device="cpu", labels=labels)
    assert ptr.dtype.is_floating_point is False and str(ptr.dtype) == "torch.int64" and str(ids.dtype) == "torch.int32"
    ptr, ids = ptr.numpy(), ids.numpy()
    want = dict_of_sets(arrays, labels)
    assert ptr.shape == (n_user + 1,) and ptr[0] == 0 and ptr[-1] == ids.size == sum(len(v) for v in want.values())
    for u in range(n_user):
        assert ids[ptr[u]:ptr[u + 1]].tolist() == sorted(want.get(u, ()))
    assert ptr[-1] == ptr[-4]                                          # the users without rows have empty rows
    one = data_prep.interaction_csr(arrays[0], n_user, device="cpu", labels=labels)      # a single array is accepted too
    w1 = dict_of_sets(arrays[:1], labels)
    assert one[1].numel() == sum(len(v) for v in w1.values())
    with pytest.raises(ValueError, match="user ids"):
        data_prep.interaction_csr(arrays, n_user - 10, device="cpu")


def oracle_stub(calls):
    """data_prep.sample_negatives with the kernel replaced by the host oracle (torch tensors on the CPU device)."""
    import torch

    def stub(excl, n_item, counts, seed=1, round=0, check=True, total=None):
        calls.append(dict(seed=seed, round=round, check=check, total=total))
        ptr, items, status = no.sample_negatives_scalar(excl[0].numpy(), excl[1].numpy(), counts.numpy(), n_item, seed, round)
        assert total == items.size
        res = (torch.from_numpy(ptr), torch.from_numpy(items), torch.from_numpy(status))
        return res if not check else res[:2]
    return stub


def test_negative_sampler_counts_layout_and_exclusion(monkeypatch):
    from mvin_amd import data_prep
    n_user, n_item = 30, 200
    train, ev, te = splits(3, n_item=n_item)
    calls = []
    monkeypatch.setattr(data_prep, "sample_negatives", oracle_stub(calls))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # nobody is clipped here: no warning
        s = data_prep.NegativeSampler(train, n_user, n_item, exclude=(ev, te), ratio=1.0, seed=9, device="cpu")
    pos = train[train[:, 2] == 1]
    n_pos_of = np.bincount(pos[:, 0], minlength=n_user)
    assert s.counts.numpy().tolist() == n_pos_of.tolist() and s.n_pos == pos.shape[0] and s.n_neg == pos.shape[0]
    rows = s.epoch(4)
    assert calls[-1] == dict(seed=9, round=4, check=False, total=s.n_neg)
    assert str(rows.dtype) == "torch.int64" and tuple(rows.shape) == (s.n_pos + s.n_neg, 3)
    rows = rows.numpy()
    assert np.array_equal(rows[:s.n_pos], pos)                        # the positives first, in train_data order
    neg = rows[s.n_pos:]
    assert (neg[:, 2] == 0).all() and (neg[:, 1] >= 0).all() and (neg[:, 1] < n_item).all()
    assert np.array_equal(neg[:, 0], np.repeat(np.arange(n_user), n_pos_of))           # user-major
    seen = dict_of_sets((train, ev, te), 1)
    for u, i, _ in neg.tolist():
        assert i not in seen.get(u, ())                               # no label-1 item of any split
    # the negatives are the rule's, in the rule's order
    ptr, ids = data_prep._interaction_csr_host([train, ev, te], n_user, 1)
    want = no.sample_negatives_scalar(ptr, ids, n_pos_of, n_item, 9, 4)[1]
    assert np.array_equal(neg[:, 1], want)
    assert not np.array_equal(s.epoch(5).numpy(), rows) and np.array_equal(s.epoch(4).numpy(), rows)


def test_negative_sampler_ratio_rounds_half_up_and_clips_with_one_warning(monkeypatch):
    from mvin_amd import data_prep
    n_user, n_item = 6, 10
    #          user: positives           (label-1 items)
    train = [(0, i, 1) for i in range(1)] + [(1, i, 1) for i in range(2)] + [(2, i, 1) for i in range(3)] \
        + [(3, i, 1) for i in range(8)] + [(4, i, 1) for i in range(5)] + [(4, 9, 0), (5, 3, 0)]
    train = np.array(train, dtype=np.int64)
    ev = np.array([(3, 8, 1), (3, 8, 1), (4, 5, 0), (4, 12, 1), (4, -2, 1)], dtype=np.int64)     # user 3: 9 excluded; out-of-range ids
    monkeypatch.setattr(data_prep, "sample_negatives", oracle_stub([]))
    with pytest.warns(UserWarning, match="2 users") as rec:
        s = data_prep.NegativeSampler(train, n_user, n_item, exclude=(ev,), ratio=1.5, seed=1, device="cpu")
    assert len([w for w in rec if "NegativeSampler" in str(w.message)]) == 1
    # round half up of 1.5 * (1, 2, 3, 8, 5, 0) = 2, 3, 5 (4.5 -> 5), 12, 8 (7.5 -> 8), 0; eligible = 9, 8, 7, 1, 5, 10
    assert no.round_half_up_counts([1, 2, 3, 8, 5, 0], 1.5).tolist() == [2, 3, 5, 12, 8, 0]
    assert s.counts.numpy().tolist() == [2, 3, 5, 1, 5, 0]
    rows = s.epoch(0).numpy()
    assert (rows[:, 1] >= 0).all()                                    # no -1 reaches the epoch tensor
    neg = rows[s.n_pos:]
    assert neg[neg[:, 0] == 3][:, 1].tolist() == [9]                   # the one item user 3 may still get
    assert sorted(neg[neg[:, 0] == 4][:, 1].tolist()) == [5, 6, 7, 8, 9]
    assert s.last_status.tolist() == [0, 0]


def test_train_rejects_unknown_negatives_mode():
    from mvin_amd import harness
    with pytest.raises(ValueError, match="negatives"):
        harness.train(None, (0,) * 10, negatives="bogus")


# --------------------------------------------------------------------------- the generated ISA
def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_both_negatives_kernels_use_no_scratch(tmp_path):
    """The one sampler source holds two instances of one kernel body, the uniform draw and the alias draw."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path / "neg.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", os.path.join(CSRC, "mvin_negatives.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S*sample_negatives_kernel\S*)\s*$(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert len(kernels) == 2 and len({name for name, _ in kernels}) == 2, [name for name, _ in kernels]
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == 2          # nothing else in the unit
    for name, body in kernels:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert seg is not None and int(seg.group(1)) == 0, name
        assert re.search(r"\.amdhsa_wavefront_size32\s+1", body) is None, name
    for key in ("vgpr_spill_count", "sgpr_spill_count"):
        found = re.findall(rf"\.{key}:\s*(\d+)", text)
        assert len(found) == 2 and all(int(v) == 0 for v in found), (key, found)
