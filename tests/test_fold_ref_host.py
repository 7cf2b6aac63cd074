"""tests/fold_ref.py -- the float64 yardstick of the folded score forms -- against two independent evaluations on a tiny instance
(CPU only): bench.l2_reference_f64 followed by the tail test's reference, and a per-pair, per-slot Python loop over the formulas of
include/mvin_hip.h."""
import math

import numpy as np
import pytest
import torch

import bench
from fold_ref import clamp_ids, fold_reference, fold_tables_reference, tail_reference
from test_gpu_tail import _reference as tail_reference_f64

D, K, N_ENTITY, NR, B = 8, 3, 11, 4, 5


def _instance(seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32) * 0.3        # noqa: E731
    ae = torch.randint(0, N_ENTITY, (N_ENTITY, K), generator=g, dtype=torch.int32)
    ar = torch.randint(0, NR, (N_ENTITY, K), generator=g, dtype=torch.int32)
    ae[2, 1], ar[2, 1] = ae[2, 0], ar[2, 0]                   # a repeated slot
    items = torch.tensor([0, 10, 2, 2, 7], dtype=torch.int64)
    w = {n: f(D, D) for n in ("W0", "W1", "W2", "A0", "A1")}
    w["Wmix"] = f(3 * D, D)
    b = {n: (f(D) if bias else None) for n in ("b0", "b1", "b2", "a0", "a1", "bmix")}
    return dict(E=f(N_ENTITY, D), ae=ae, ar=ar, items=items, t0=f(NR) * 3, t1=f(NR) * 3, q=f(B, D), uo=f(B, D), **w, **b)


def _call(c, t0, t1, dtype=torch.float64, items=None):
    return fold_reference(c["E"], c["ae"], c["ar"], c["items"] if items is None else items, t0, t1, c["q"], c["uo"], c["W0"], c["b0"], c["W1"],
                          c["b1"], c["W2"], c["b2"], c["A0"], c["a0"], c["A1"], c["a1"], c["Wmix"], c["bmix"], K, dtype=dtype)


def _naive(c, t0, t1):
    """One pair, one slot, one column at a time (float64 Python floats through numpy rows)."""
    n = lambda t: None if t is None else t.double().numpy()   # noqa: E731
    E, ae, ar, q, uo = n(c["E"]), c["ae"].numpy(), c["ar"].numpy(), n(c["q"]), n(c["uo"])
    W0, W1, W2, A0, A1, Wmix = (n(c[k]) for k in ("W0", "W1", "W2", "A0", "A1", "Wmix"))
    zero = np.zeros(D)
    b0, b1, b2, a0, a1, bmix = (zero if c[k] is None else n(c[k]) for k in ("b0", "b1", "b2", "a0", "a1", "bmix"))
    t0, t1 = n(t0), n(t1)

    def weights(t, rels):
        if t is None:
            return [1.0] * len(rels)
        m = max(t[r] for r in rels)
        e = [math.exp(t[r] - m) for r in rels]
        return [v / sum(e) for v in e]

    relu = lambda v: np.maximum(v, 0.0)                       # noqa: E731
    out = []
    for i, x in enumerate(c["items"].tolist()):
        nagg0, nagg1 = np.zeros(D), np.zeros(D)
        p0, p1 = weights(t0, ar[x]), weights(t1, ar[x])
        for s in range(K):
            ch = ae[x, s]
            p = weights(t0, ar[ch])
            self1 = (E[ch] + q[i]) @ W1 + b1
            neigh = np.zeros(D)
            for k in range(K):
                neigh += p[k] * ((E[ae[ch, k]] + q[i]) @ W2 + b2)
            out1 = relu((self1 + neigh / K) @ A0 + a0)
            nagg0 += p0[s] * self1 / K
            nagg1 += p1[s] * out1 / K
        ev0 = (E[x] + q[i]) @ W0 + b0
        out0 = relu((ev0 + nagg0) @ A0 + a0)
        out2 = relu((out0 + nagg1) @ A1 + a1)
        item = np.concatenate([ev0, out0, out2]) @ Wmix + bmix
        s_ = float(uo[i] @ item)
        out.append((nagg0, nagg1, item, s_, 1.0 / (1.0 + math.exp(-s_))))
    return [np.stack([o[j] for o in out]) for j in range(5)]


def test_equals_the_two_references_it_composes():
    c = _instance(1)
    n0, n1, item, s, sg = _call(c, c["t0"], c["t1"])
    r0, r1 = bench.l2_reference_f64(c["E"], c["ae"], c["ar"], c["items"], c["t0"], c["t1"], c["W1"], c["W2"], c["b1"], c["b2"], c["q"], c["A0"], c["a0"], K)
    ri, rs, rg = tail_reference_f64(c["E"], c["items"], c["q"], c["uo"], r0, r1, c["W0"], c["b0"], c["A0"], c["a0"], c["A1"], c["a1"], c["Wmix"], c["bmix"])
    for got, want in ((n0, r0), (n1, r1), (item, ri), (s, rs), (sg, rg)):
        assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("bias", [True, False], ids=["biases", "no-biases"])
def test_tail_reference_without_the_projection(bias):
    """W0 = None (User_orient off): ev0 = E[x], q and b0 unused -- against plain torch float64 ops, and in its fp32 evaluation."""
    c = _instance(6, bias)
    d = lambda t: 0 if t is None else t.double()              # noqa: E731
    x = torch.tensor([0, 10, 2, 2, 7])
    n0, n1 = c["q"] * 0.5 + 0.1, c["uo"] * 0.7 - 0.2         # any [B, D] rows
    ev0 = c["E"].double()[x]
    out0 = torch.relu((ev0 + n0.double()) @ c["A0"].double() + d(c["a0"]))
    out2 = torch.relu((out0 + n1.double()) @ c["A1"].double() + d(c["a1"]))
    item = ev0 @ c["Wmix"][:D].double() + out0 @ c["Wmix"][D:2 * D].double() + out2 @ c["Wmix"][2 * D:].double() + d(c["bmix"])
    s = (c["uo"].double() * item).sum(1)
    tail = (c["A0"], c["a0"], c["A1"], c["a1"], c["Wmix"], c["bmix"])
    for q, b0 in ((None, None), (c["q"], c["b0"])):           # neither may enter
        got = tail_reference(c["E"], x, q, c["uo"], n0, n1, None, b0, *tail)
        for g_, w_ in zip(got, (item, s, torch.sigmoid(s))):
            assert g_.dtype == torch.float64 and float((g_ - w_).abs().max()) <= 1e-12
    with_w0 = tail_reference(c["E"], x, c["q"], c["uo"], n0, n1, c["W0"], c["b0"], *tail)
    assert float((with_w0[0] - item).abs().max()) > 1e-3      # ... and the projection does change the result
    lo = tail_reference(c["E"], x, None, c["uo"], n0, n1, None, None, *tail, dtype=torch.float32)
    assert all(t.dtype == torch.float32 for t in lo) and 0 < float((lo[0].double() - item).abs().max()) < 1e-5


@pytest.mark.parametrize("bias", [True, False], ids=["biases", "no-biases"])
@pytest.mark.parametrize("att", ["both", "none", "t0", "t1"])
def test_equals_a_naive_loop(att, bias):
    c = _instance(2, bias)
    t0 = c["t0"] if att in ("both", "t0") else None
    t1 = c["t1"] if att in ("both", "t1") else None
    got = _call(c, t0, t1)
    want = _naive(c, t0, t1)
    for g_, w_, nm in zip(got, want, ("nagg0", "nagg1", "item_emb", "scores", "sigmoid")):
        assert np.abs(g_.numpy() - w_).max() <= 1e-12, nm
    if att == "none":                                         # the plain mean, not a softmax of zeros over K
        zeros = torch.zeros(NR)
        assert float((_call(c, zeros, zeros)[3] - got[3]).abs().max()) > 1e-6


def test_ids_are_clamped_as_unsigned_words():
    c = _instance(3)
    bad = torch.tensor([N_ENTITY + 12345, 10, -1, 2, (1 << 32) + 4], dtype=torch.int64)
    assert clamp_ids(bad, N_ENTITY).tolist() == [10, 10, 10, 2, 4]
    assert clamp_ids(torch.tensor([-1, 3], dtype=torch.int32), N_ENTITY).tolist() == [10, 3]
    a = _call(c, c["t0"], c["t1"], items=bad)
    b = _call(c, c["t0"], c["t1"], items=torch.tensor([10, 10, 10, 2, 4]))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_float32_evaluation_is_float32_and_close():
    c = _instance(4)
    lo, hi = _call(c, c["t0"], c["t1"], dtype=torch.float32), _call(c, c["t0"], c["t1"])
    for x, y in zip(lo, hi):
        assert x.dtype == torch.float32
        err = float((x.double() - y).abs().max())
        assert 0 < err < 1e-5


def test_table_definitions_fold_back_into_the_pair_formulas():
    """H0 | G | M0 (fold_tables_reference) recombined as the header folds them give the reference's item embeddings."""
    c = _instance(5)
    d = lambda t: t.double()                                  # noqa: E731
    T = fold_tables_reference(c["E"], c["ae"], c["ar"], c["t0"], c["W0"], c["W1"], c["W2"], c["A0"], c["Wmix"], K)
    x = c["items"]
    cK = 1.0 / K
    q = d(c["q"])
    Wm0, Wm1, Wm2 = d(c["Wmix"][:D]), d(c["Wmix"][D:2 * D]), d(c["Wmix"][2 * D:])
    out0 = torch.relu(T["H0"][x] + q @ ((d(c["W0"]) + cK * d(c["W1"])) @ d(c["A0"])) + (d(c["b0"]) + cK * d(c["b1"])) @ d(c["A0"]) + d(c["a0"]))
    v = q @ ((d(c["W1"]) + cK * d(c["W2"])) @ d(c["A0"])) + (d(c["b1"]) + cK * d(c["b2"])) @ d(c["A0"]) + d(c["a0"])
    p1 = torch.softmax(d(c["t1"])[c["ar"][x].long()], dim=-1) / K
    z2 = out0 + (p1[..., None] * torch.relu(T["G"][c["ae"][x].long()] + v[:, None, :])).sum(1)
    out2 = torch.relu(z2 @ d(c["A1"]) + d(c["a1"]))
    item = T["M0"][x] + q @ d(c["W0"]) @ Wm0 + d(c["b0"]) @ Wm0 + out0 @ Wm1 + out2 @ Wm2 + d(c["bmix"])
    assert float((item - _call(c, c["t0"], c["t1"])[2]).abs().max()) <= 1e-12
