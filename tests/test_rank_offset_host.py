"""CPU: the logQ-corrected sampled softmax (mvin_rank_head_offset, NegativeSampler.log_proposal, data_prep.rank_offsets,
Trainer.set_objective(offset=True), harness.train(logq=True)) as far as it goes without a GPU: the C ABI's symbol and argument
validation (nothing is launched), the proposal and the offsets of a 6-item catalogue against numbers written out here, the
identity the correction rests on by exact enumeration, the float64 reference of tests/rank_offset_ref.py against autograd,
and the argument errors of ``train`` and ``Trainer``."""
import ctypes as C
import math
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

import rank_loss_ref as rl
import rank_offset_ref as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the C ABI (nothing is launched)
def test_symbol_declared_exported_and_bound(hip_lib):
    from mvin_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvin_hip.h")).read(), flags=re.S)
    assert "mvin_rank_head_offset" in set(re.findall(r"\b(mvin_[a-z0-9_]+)\s*\(", src))
    assert hasattr(hip_lib, "mvin_rank_head_offset")
    vmap = open(os.path.join(ROOT, "mvin_amd", "csrc", "libmvin_hip.map")).read()
    assert re.search(r"global:\s*mvin_\*;", vmap) and "mvin_rank_head_offset" in vmap
    res, argtypes = _lib.SIGNATURES["mvin_rank_head_offset"]
    base_res, base_args = _lib.SIGNATURES["mvin_rank_head"]
    assert res is C.c_int and len(argtypes) == 16
    assert base_res is C.c_int and len(base_args) == 15                  # mvin_rank_head keeps its signature
    assert list(argtypes[:3]) == list(base_args[:3]) and list(argtypes[4:]) == list(base_args[3:])      # + offset after valid
    assert hip_lib.mvin_abi_version() == 12
    decl = re.search(r"int\s+mvin_rank_head\s*\(([^)]*)\)", src).group(1)
    assert "offset" not in decl and decl.count(",") == 14
    decl_off = re.search(r"int\s+mvin_rank_head_offset\s*\(([^)]*)\)", src).group(1)
    assert "const float* offset" in decl_off and decl_off.count(",") == 15


def test_argument_errors_return_codes_and_launch_nothing(hip_lib):
    """Null or dummy pointers only: a call that got past validation would fault on them."""
    one = C.c_void_p(16)
    f = hip_lib.mvin_rank_head_offset

    def call(ptrs=None, n_groups=3, G=4, D=8, mode=0, offset=one):
        p = ptrs or [one] * 7          # user_o, item_emb, scores, dscore, du, di, loss_accum
        rc = f(p[0], p[1], None, offset, n_groups, G, D, mode, 1.0, p[2], p[3], p[4], p[5], p[6], None, None)
        return rc, hip_lib.mvin_last_error()

    for offset in (one, None):         # the offset itself may be NULL: it is never the reason of a -1
        for hole in range(7):
            ptrs = [one] * 7
            ptrs[hole] = None
            rc, msg = call(ptrs, offset=offset)
            assert rc == -1 and b"mvin_rank_head_offset" in msg and b"null" in msg, (hole, rc, msg)
        for G in (1, 0, -2, 65):
            rc, msg = call(G=G, offset=offset)
            assert rc == -2 and b"mvin_rank_head_offset" in msg and b"G=%d" % G in msg
        for D in (6, 0, 2, 132, 256, -8):
            rc, msg = call(D=D, offset=offset)
            assert rc == -2 and b"D=%d" % D in msg
        for mode in (2, -1):
            rc, msg = call(mode=mode, offset=offset)
            assert rc == -2 and b"mode=%d" % mode in msg
        rc, msg = call(n_groups=-1, offset=offset)
        assert rc == -2 and b"n_groups=-1" in msg
        assert call(n_groups=0, offset=offset)[0] == 0                   # nothing to do, nothing launched
    # the messages of the old entry point still carry its own name
    rc = hip_lib.mvin_rank_head(None, one, None, 3, 4, 8, 0, 1.0, one, one, one, one, one, None, None)
    msg = hip_lib.mvin_last_error()
    assert rc == -1 and b"mvin_rank_head:" in msg and b"offset" not in msg


def test_ops_wrapper_checks_before_the_call():
    from mvin_amd import _lib, ops
    with pytest.raises(ValueError, match="mode"):
        ops.rank_head(None, None, 2, "hinge", 1.0, None, offset=torch.zeros(4))
    with pytest.raises(_lib.MvinHipError, match="no CPU path"):
        ops.rank_head(torch.zeros(4, 8), torch.zeros(4, 8), 2, "bpr", 1.0, torch.zeros(1), offset=torch.zeros(4))


# --------------------------------------------------------------------------- the proposal and the offsets by hand
N_USER, N_ITEM = 2, 6
#   user 0: positives 0, 1 in train, 3 in eval           -> exclusion row {0, 1, 3}
#   user 1: positive 2 in train, the out-of-range id 9    -> exclusion row {2, 9}: one in-range id
TRAIN = np.array([(0, 0, 1), (0, 1, 1), (1, 2, 1), (1, 5, 0)], dtype=np.int64)
EVAL = np.array([(0, 3, 1), (1, 9, 1)], dtype=np.int64)
WEIGHTS = np.array([4.0, 2.0, 1.0, 0.0, 1.0, 2.0])         # item 3 is masked; p = w / 10 up to the table's 2^-32 steps
# hand-made groups in the layout of rank_groups (n_neg = 2): full, clipped to one negative, none, full
USERS = torch.tensor([0, 0, 1, 1], dtype=torch.int64)
ITEMS = torch.tensor([[0, 2, 4], [1, 5, 3], [2, 2, 2], [2, 0, 1]], dtype=torch.int64)      # [1, 2] holds the MASKED item, invalid
VALID = torch.tensor([[1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 1, 1]], dtype=torch.float32)


def make_sampler(weighted):
    from mvin_amd import data_prep
    kw = {"weights": WEIGHTS} if weighted else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # user 0 is clipped: 4 negatives wanted, 3 (2 weighted) eligible
        return data_prep.NegativeSampler(TRAIN, N_USER, N_ITEM, exclude=(EVAL,), ratio=2.0, seed=3, device="cpu", **kw)


def test_log_proposal_uniform_by_hand():
    s = make_sampler(False)
    assert s.eligible_host.tolist() == [3, 5]              # c_u: 6 - {0, 1, 3}; 6 - {2} (9 is out of range)
    logp, logmass = s.log_proposal()
    assert logp.dtype == logmass.dtype == torch.float32 and tuple(logp.shape) == (6,) and tuple(logmass.shape) == (2,)
    assert logp.tolist() == [float(np.float32(math.log(1.0 / 6.0)))] * 6
    np.testing.assert_allclose(logmass.numpy(), np.float32([math.log(3.0 / 6.0), math.log(5.0 / 6.0)]), rtol=0, atol=2.0 ** -24)
    np.testing.assert_allclose(torch.exp(logmass.double()).numpy() * 6, s.eligible_host, rtol=1e-7)
    again = s.log_proposal()
    assert again[0] is logp and again[1] is logmass        # computed once, cached


def test_log_proposal_weighted_by_hand():
    from mvin_amd import data_prep
    s = make_sampler(True)
    #   user 0: 6 - {0, 1, 3} = {2, 4, 5}: the masked item 3 is in the row too and is counted out ONCE
    #   user 1: 6 - {2} - the masked {3} = {0, 1, 4, 5}
    assert s.eligible_host.tolist() == [3, 4]
    tab, mask = data_prep.alias_table(WEIGHTS, N_ITEM)
    p = data_prep.alias_probabilities(tab)
    np.testing.assert_allclose(p, WEIGHTS / 10.0, rtol=0, atol=1e-8)
    logp, logmass = s.log_proposal()
    assert logp[3].item() == float("-inf")                 # the masked item
    live = [0, 1, 2, 4, 5]
    np.testing.assert_allclose(torch.exp(logp.double()).numpy()[live], p[live], rtol=2.0 ** -22, atol=0)
    np.testing.assert_allclose(torch.exp(logp.double()).numpy()[live], [0.4, 0.2, 0.1, 0.1, 0.2], rtol=1e-6)
    mass = [p[2] + p[4] + p[5], p[0] + p[1] + p[4] + p[5]]                 # user 0: {2, 4, 5}; user 1: {0, 1, 4, 5}
    np.testing.assert_allclose(torch.exp(logmass.double()).numpy(), mass, rtol=2.0 ** -22)
    np.testing.assert_allclose(torch.exp(logmass.double()).numpy(), [0.4, 0.9], rtol=1e-6)
    p_np, mass_np, count_np = ro.log_proposal_np(s)
    np.testing.assert_allclose(p_np, np.where(np.arange(6) == 3, 0.0, p), rtol=0, atol=0)
    np.testing.assert_allclose(mass_np, mass, rtol=1e-15)
    assert count_np.tolist() == s.eligible_host.tolist()


def test_rank_offsets_by_hand():
    from mvin_amd import data_prep
    for weighted in (False, True):
        s = make_sampler(weighted)
        off = data_prep.rank_offsets(s, USERS, ITEMS, VALID)
        assert off.dtype == torch.float32 and tuple(off.shape) == (4, 3) and off.is_contiguous()
        o = off.numpy()
        assert not o[:, 0].any() and not o[VALID.numpy() == 0].any()       # slot 0 and invalid slots: exactly 0
        assert np.isfinite(o).all()                                         # the -inf of the masked item in [1, 2] went nowhere
        if not weighted:                                                    # log(n_g / c_u), c = (3, 5)
            want = {(0, 1): math.log(2 / 3), (0, 2): math.log(2 / 3), (1, 1): math.log(1 / 3), (3, 1): math.log(2 / 5),
                    (3, 2): math.log(2 / 5)}
            for k, w in want.items():
                assert o[k] == np.float32(w), (k, o[k], w)
        else:                                                               # log(n_g p / mass), p = w / 10, mass = (.4, .9)
            want = {(0, 1): math.log(2 * 0.1 / 0.4), (0, 2): math.log(2 * 0.1 / 0.4), (1, 1): math.log(1 * 0.2 / 0.4),
                    (3, 1): math.log(2 * 0.4 / 0.9), (3, 2): math.log(2 * 0.2 / 0.9)}
            for k, w in want.items():
                assert abs(o[k] - w) <= 1e-6, (k, o[k], w)
        assert np.array_equal(o, ro.rank_offsets_np(s, USERS, ITEMS, VALID)) or \
            np.abs(o - ro.rank_offsets_np(s, USERS, ITEMS, VALID)).max() <= 2.0 ** -23       # one float32 rounding of O(1) values


# --------------------------------------------------------------------------- the identity the correction rests on
def test_corrected_one_draw_partition_is_unbiased_by_enumeration():
    """12 items, a skewed proposal, float64, no sampling: E_j~q_u [ e^{s_j} / q_u(j) ] = sum over the eligible items of e^{s_j},
    so the corrected one-draw group's Z has the full partition (positive + eligible) as its expectation; uncorrected it has not."""
    rng = np.random.default_rng(5)
    n = 12
    p = 1.0 / np.arange(1, n + 1) ** 1.2
    p /= p.sum()
    s = rng.normal(size=n) * 2.0
    positive, excluded = 3, {3, 0, 7}                       # the user's row: the positive and two more watched items
    elig = [j for j in range(n) if j not in excluded]
    mass = math.fsum(p[j] for j in elig)
    q = {j: p[j] / mass for j in elig}
    assert math.isclose(math.fsum(q.values()), 1.0, rel_tol=1e-15)
    full = math.exp(s[positive]) + math.fsum(math.exp(s[j]) for j in elig)
    for mode_offset in (True, False):
        expect = 0.0
        for j in elig:                                      # the one-draw group (positive | j), n_g = 1: offset = log q_u(j)
            off = np.array([0.0, math.log(1 * p[j] / mass)]) if mode_offset else None
            ref = ro.rank_head_offset_ref(np.array([s[positive], s[j]]), None, off, 2, "softmax")
            Z = math.exp(float(ref.loss_groups[0]) + s[positive])          # l = log Z - z_0 and z_0 = s_0
            expect += q[j] * Z
        if mode_offset:
            assert math.isclose(expect, full, rel_tol=1e-12), (expect, full)
        else:
            plain = math.exp(s[positive]) + math.fsum(q[j] * math.exp(s[j]) for j in elig)
            assert math.isclose(expect, plain, rel_tol=1e-12)
            assert abs(expect - full) > 0.1 * full          # not the partition function ...
            ratio = (expect - math.exp(s[positive])) / (full - math.exp(s[positive]))
            assert abs(ratio * len(elig) - 1.0) > 0.05      # ... nor a catalogue-size multiple of its negative part


# --------------------------------------------------------------------------- the float64 reference with offsets
def random_case(rng, n_g, G, scale=3.0, p_valid=0.7):
    s = rng.normal(size=n_g * G) * scale
    valid = (rng.random(n_g * G) < p_valid).astype(np.float32)
    valid.reshape(n_g, G)[:, 0] = 0.0                      # the flag of slot 0 is ignored: it always counts
    off = rng.normal(size=n_g * G) * 4.0 - 3.0             # slot 0 carries one too: the kernel's contract covers it
    return s, valid, off


@pytest.mark.parametrize("mode", ro.MODES)
@pytest.mark.parametrize("G", [2, 3, 5, 33, 64])
def test_reference_with_offsets_agrees_with_autograd(mode, G):
    rng = np.random.default_rng(G)
    for valid_kind in ("none", "random", "all_masked"):
        s, valid, off = random_case(rng, 9, G)
        if valid_kind == "none":
            valid = None
        elif valid_kind == "all_masked":
            valid.reshape(9, G)[::2, 1:] = 0.0
        ref = ro.rank_head_offset_ref(s, valid, off, G, mode)
        t = torch.tensor(s, dtype=torch.float64, requires_grad=True)
        lg = ro.rank_head_offset_torch(t, valid, off, G, mode)
        lg.sum().backward()
        np.testing.assert_allclose(ref.loss_groups, lg.detach().numpy(), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(ref.dscore, t.grad.numpy(), rtol=1e-13, atol=1e-14)
        mask = rl.valid_mask(valid, 9, G).reshape(-1)
        assert not ref.dscore[~mask].any()
        assert np.array_equal(ref.scores, s) and ref.counts == rl.pair_counts(s, valid, G)       # raw scores, raw counts
        # the offsets do something, and those of invalid slots do nothing -- whatever they hold
        base = rl.rank_head_ref(s, valid, G, mode)
        assert not np.allclose(ref.loss_groups[base.loss_groups != 0], base.loss_groups[base.loss_groups != 0])
        poisoned = off.copy()
        poisoned[~mask] = np.nan
        again = ro.rank_head_offset_ref(s, valid, poisoned, G, mode)
        assert np.array_equal(again.dscore, ref.dscore) and np.array_equal(again.loss_groups, ref.loss_groups)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ro.MODES)
def test_offset_zero_is_the_reference_without_offsets(mode, dtype):
    rng = np.random.default_rng(11)
    s, valid, _ = random_case(rng, 13, 5, scale=8.0)
    for off in (None, np.zeros(65)):
        a = ro.rank_head_offset_ref(s, valid, off, 5, mode, dtype=dtype)
        b = rl.rank_head_ref(s, valid, 5, mode, dtype=dtype)
        for k in ("scores", "loss_groups", "dscore"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.loss == b.loss and a.counts == b.counts


def test_bpr_offset_is_a_margin():
    s = np.array([1.0, 0.5, 2.0])
    off = np.array([0.25, -1.0, 0.5])
    ref = ro.rank_head_offset_ref(s, None, off, 3, "bpr")
    x = np.array([(0.5 + 1.0) - (1.0 - 0.25), (2.0 - 0.5) - (1.0 - 0.25)])
    assert math.isclose(ref.loss_groups[0], float(np.log1p(np.exp(x)).mean()), rel_tol=1e-14)


# --------------------------------------------------------------------------- argument errors of train and Trainer
def test_train_refuses_logq_where_it_does_not_apply():
    from mvin_amd import harness
    args = types.SimpleNamespace(batch_size=8)
    data = (0,) * 10
    for objective in ("bce", "bpr"):
        for negatives in ("fixed", "resample", "hard"):
            with pytest.raises(ValueError, match="logq=True.*softmax"):
                harness.train(args, data, objective=objective, negatives=negatives, logq=True)
    with pytest.raises(ValueError, match="logq=True.*fixed"):
        harness.train(args, data, objective="softmax", negatives="fixed", logq=True)
    with pytest.raises(ValueError, match="logq=True.*hard"):
        harness.train(args, data, objective="softmax", negatives="hard", n_neg=2, pool=4, logq=True)
    with pytest.raises(ValueError, match="logq"):
        harness.train(args, data, objective="softmax", negatives="resample", logq=1)


def test_trainer_offset_flag():
    from mvin_amd.training import Trainer
    tr = Trainer.__new__(Trainer)                                       # set_objective touches no device state
    tr.set_objective("softmax", 5)
    assert tr.logit_offset is False and tr.head_key() == ("softmax", 5, False)
    tr.set_objective("softmax", 5, offset=True)
    assert tr.logit_offset is True and tr.head_key() == ("softmax", 5, True)
    tr.set_objective("bpr", 3, offset=True)                             # the kernel's margin is reachable from the trainer
    assert tr.head_key() == ("bpr", 3, True)
    with pytest.raises(ValueError, match="offset"):
        tr.set_objective("bce", offset=True)
    with pytest.raises(ValueError, match="offset"):
        tr.set_objective("softmax", 5, offset="yes")
    assert tr.head_key() == ("bpr", 3, True)                            # a refused call changes nothing
    tr.set_objective("bce")
    assert tr.head_key() == ("bce", None, False)
