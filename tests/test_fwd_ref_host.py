"""CPU: tests/fwd_ref.py (the float64 contracts tests/test_gpu_fwd_kernels.py holds the forward kernels to) pinned to
independent statements of the same formulas in plain torch float64 ops (embedding, matmul, softmax), row by row where the
contract has strides or groups.  For the aggregator also the un-reassociated form of the header comment,
reduce_mean_k(p_k * ((table[y_k] + q) . W + b)), so that the linearity step is checked and not assumed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_ref

T64 = torch.float64


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def tid(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64))


def close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), want.numpy().reshape(np.shape(got)), rtol=1e-12, atol=1e-12, err_msg=what)


# ----------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("sum_sources", [False, True])
@pytest.mark.parametrize("ids64", [False, True])
def test_linear_every_field(sum_sources, ids64):
    rng = np.random.default_rng(1)
    rows, Dsrc, Dout, nz, nsrc, ntab, rpg = 11, 8, 5, 3, 3, 6, 4
    Din = Dsrc if sum_sources else nsrc * Dsrc
    srcs = [rng.standard_normal((ntab, Dsrc)), rng.standard_normal((rows + 2, Dsrc)), rng.standard_normal((ntab, Dsrc))]
    ids = [rng.integers(-3, ntab + 3, rows).astype(np.int64 if ids64 else np.int32), None,
           rng.integers(0, ntab, rows).astype(np.int64 if ids64 else np.int32)]
    ids[0][:3] = (-1, ntab, 2 ** 31 - 1)
    wzs, bzs, ozs, ldo, off = Din * Dout + 3, Dout + 1, rows * 9 + 5, 9, 2
    W, bias = rng.standard_normal(nz * wzs), rng.standard_normal(nz * bzs)
    rowbias = rng.standard_normal(((rows + rpg - 1) // rpg, Dout))
    pre = rng.standard_normal(off + nz * ozs)
    got = fwd_ref.linear(srcs, W, Dout, rows=rows, ids=ids, bias=bias, rowbias=rowbias, rows_per_group=rpg, relu=True,
                         sum_sources=sum_sources, nz=nz, w_zstride=wzs, bias_zstride=bzs, src_rows=ntab, out=pre,
                         out_offset=off, ldo=ldo, out_zstride=ozs)
    # independent: embedding lookups with the clamp written out, torch.cat / sum, matmul
    cl = [None if i is None else torch.where((tid(i) < 0) | (tid(i) >= ntab), torch.tensor(ntab - 1), tid(i)) for i in ids]
    parts = [t64(s)[:rows] if i is None else F.embedding(i, t64(s)) for s, i in zip(srcs, cl)]
    X = torch.stack(parts).sum(0) if sum_sources else torch.cat(parts, dim=1)
    flat = t64(pre).clone()
    for z in range(nz):
        Wz = t64(W)[z * wzs:z * wzs + Din * Dout].view(Din, Dout)
        y = torch.relu(torch.matmul(X, Wz) + t64(bias)[z * bzs:z * bzs + Dout] + t64(rowbias)[torch.arange(rows) // rpg])
        close(got["out"][z], y, f"out[{z}]")
        for r in range(rows):
            flat[off + z * ozs + r * ldo: off + z * ozs + r * ldo + Dout] = y[r]
    close(got["flat"], flat, "flat buffer")
    assert got["score"] is None and got["sigmoid"] is None
    # the negative id and the ids past the end read the LAST row
    assert torch.equal(parts[0][:3], t64(srcs[0])[ntab - 1].expand(3, Dsrc))


def test_linear_score_sigmoid_identity_and_no_clamp():
    rng = np.random.default_rng(2)
    rows, D = 7, 8
    src, W, u = rng.standard_normal((rows, D)), rng.standard_normal((D, D + 4)), rng.standard_normal((rows, D + 4))
    got = fwd_ref.linear([src], W, D + 4, rows=rows, score_u=u)
    y = torch.matmul(t64(src), t64(W))
    sc = (y * t64(u)).sum(1)
    close(got["out"][0], y, "out")
    close(got["score"], sc, "score")
    close(got["sigmoid"], torch.sigmoid(sc), "sigmoid")
    # identity copy, gathered, src_rows = 0: ids used as they are
    ids = rng.integers(0, rows, 5).astype(np.int32)
    got = fwd_ref.linear([src], None, D, rows=5, ids=[ids], bias=np.ones(D))
    close(got["out"][0], F.embedding(tid(ids), t64(src)) + 1.0, "identity copy")
    # identity over summed sources
    got = fwd_ref.linear([src, 2 * src], None, D, rows=rows, sum_sources=True)
    close(got["out"][0], 3 * t64(src), "identity over a sum")


def test_linear_magnitude_bounds_the_value():
    rng = np.random.default_rng(3)
    rows, D = 9, 8
    src, W, b, rb, u = (rng.standard_normal(s) for s in ((rows, D), (2 * D, D), (D,), (rows, D), (rows, D)))
    kw = dict(rows=rows, bias=b, rowbias=rb, score_u=u)
    val, mag = fwd_ref.linear([src, src], W, D, **kw), fwd_ref.linear([src, src], W, D, magnitude=True, **kw)
    X = torch.cat([t64(src), t64(src)], 1).abs()
    close(mag["out"][0], torch.matmul(X, t64(W).abs()) + t64(b).abs() + t64(rb).abs(), "magnitude")
    assert np.all(np.abs(val["out"]) <= mag["out"]) and np.all(np.abs(val["score"]) <= mag["score"])
    # ReLU is left out of the magnitude
    assert np.array_equal(fwd_ref.linear([src, src], W, D, relu=True, magnitude=True, **kw)["out"], mag["out"])


# ----------------------------------------------------------------------------------------------- aggregator
def _agg_inputs(rng, B, N, K, D, nE, nR):
    T = B * N
    return dict(table=rng.standard_normal((nE, D)), adj_e=rng.integers(0, nE, (nE, K)), adj_r=rng.integers(0, nR, (nE, K)),
                node=rng.integers(0, nE, T), t=rng.standard_normal(nR) * 3, self_vec=rng.standard_normal((T, D)),
                Wc=rng.standard_normal((D, D)), q=rng.standard_normal((B, D)), bL=rng.standard_normal(D),
                Wagg=rng.standard_normal((D, D)), bagg=rng.standard_normal(D))


@pytest.mark.parametrize("attention", [True, False])
def test_agg_gather_is_the_unreassociated_reduce_mean(attention):
    """reduce_mean_k(p_k * ((table[y_k] + q_b) . W_L + b_L)) with c_child = q_b . W_L + b_L."""
    rng = np.random.default_rng(4)
    B, N, K, D, nE, nR = 3, 3, 5, 8, 17, 4
    i = _agg_inputs(rng, B, N, K, D, nE, nR)
    c_child = i["q"] @ i["Wc"] + i["bL"]
    got = fwd_ref.agg(i["self_vec"], i["Wagg"], i["bagg"], K, table=i["table"], adj_entity=i["adj_e"],
                      adj_relation=i["adj_r"], node_ids=i["node"], rel_score=i["t"] if attention else None, Wc=i["Wc"],
                      c_child=c_child, N=N)
    y = F.embedding(tid(i["node"]), tid(i["adj_e"]))                                 # [T, K]
    r = F.embedding(tid(i["node"]), tid(i["adj_r"]))
    p = torch.softmax(t64(i["t"])[r], dim=1) if attention else torch.ones(B * N, K, dtype=T64)
    q = t64(i["q"]).repeat_interleave(N, 0)[:, None, :]                              # pair b of task t = t // N
    proj = torch.matmul(F.embedding(y, t64(i["table"])) + q, t64(i["Wc"])) + t64(i["bL"])      # [T, K, D]
    aggv = (p[:, :, None] * proj).mean(dim=1)
    Z = t64(i["self_vec"]) + aggv
    close(got["Z"], Z, "Z")
    close(got["out"], torch.relu(torch.matmul(Z, t64(i["Wagg"])) + t64(i["bagg"])), "out")
    close(got["S"], (p[:, :, None] * F.embedding(y, t64(i["table"]))).sum(1) / K, "S")
    if attention:
        close(got["probs"], p, "probs")
    else:
        assert got["probs"] is None


def test_agg_dense_forms():
    rng = np.random.default_rng(5)
    B, N, K, D, nR = 2, 3, 4, 8, 5
    T = B * N
    child, rel = rng.standard_normal((T * K, D)), rng.integers(0, nR, T * K)
    sv, Wagg, t = rng.standard_normal((T, D)), rng.standard_normal((D, D)), rng.standard_normal(nR)
    c = t64(child).view(T, K, D)
    for form in ("ids", "per_child", "mean"):
        if form == "ids":
            got = fwd_ref.agg(sv, Wagg, None, K, child=child, rel_ids=rel, rel_score=t)
            p = torch.softmax(t64(t)[tid(rel)].view(T, K), 1)
        elif form == "per_child":
            lg = rng.standard_normal(T * K)
            got = fwd_ref.agg(sv, Wagg, None, K, child=child, rel_score=lg)
            p = torch.softmax(t64(lg).view(T, K), 1)
        else:
            got = fwd_ref.agg(sv, Wagg, None, K, child=child)
            p = torch.ones(T, K, dtype=T64)
        S = (p[:, :, None] * c).sum(1) / K
        close(got["S"], S, form + " S")
        close(got["Z"], t64(sv) + S, form + " Z")
        close(got["out"], torch.relu(torch.matmul(t64(sv) + S, t64(Wagg))), form + " out")
    # Wc without c_child: the psum term is absent
    Wc = rng.standard_normal((D, D))
    got = fwd_ref.agg(sv, Wagg, None, K, child=child, rel_ids=rel, rel_score=t, Wc=Wc)
    p = torch.softmax(t64(t)[tid(rel)].view(T, K), 1)
    close(got["Z"], t64(sv) + torch.matmul((p[:, :, None] * c).sum(1), t64(Wc)) / K, "Wc alone")
    mag = fwd_ref.agg(sv, Wagg, None, K, child=child, rel_ids=rel, rel_score=t, Wc=Wc, magnitude=True)
    for k in ("out", "S", "Z"):
        assert np.all(np.abs(got[k]) <= mag[k] * (1 + 1e-12))


# ----------------------------------------------------------------------------------------------- ripple / small kernels
@pytest.mark.parametrize("mode", [0, 1])
def test_ripple_attn(mode):
    rng = np.random.default_rng(6)
    B, Nm, D, nE, nR = 4, 7, 8, 13, 3
    E, V, w = rng.standard_normal((nE, D)), rng.standard_normal((B, nR, D)), rng.standard_normal(3 * D)
    sid, vid, rid = rng.integers(0, nE, (B, Nm)), rng.integers(0, nE, (B, Nm)), rng.integers(0, nR, (B, Nm))
    got = fwd_ref.ripple_attn(E, sid, vid, mode, rel_ids=rid, V=V, w=w, nR=nR)
    h = F.embedding(tid(sid), t64(E))
    if mode == 0:
        v = torch.stack([F.embedding(tid(rid[b]), t64(V[b])) for b in range(B)])
        s = (h * v).sum(-1)
    else:
        s = torch.matmul(h, t64(w)[:D])
    p = torch.softmax(s, dim=1)
    close(got["probs"], p, "probs")
    close(got["o"], torch.matmul(p[:, None, :], F.embedding(tid(vid), t64(E)))[:, 0], "o")
    mag = fwd_ref.ripple_attn(E, sid, vid, mode, rel_ids=rid, V=V, w=w, nR=nR, magnitude=True)
    assert np.all(np.abs(got["o"]) <= mag["o"] * (1 + 1e-12))


def test_rel_score_and_expand_ids():
    rng = np.random.default_rng(7)
    nR, D, nE, K, B = 5, 8, 11, 3, 6
    rel, w = rng.standard_normal((nR, D)), rng.standard_normal((3 * D, 1))
    close(fwd_ref.rel_score(rel, w), torch.matmul(t64(rel), t64(w)[D:2 * D, 0]), "rel_score")
    close(fwd_ref.rel_score(rel, w, magnitude=True), torch.matmul(t64(rel).abs(), t64(w).abs()[D:2 * D, 0]), "magnitude")
    adj_e, adj_r = rng.integers(0, nE, (nE, K)), rng.integers(0, 4, (nE, K))
    items = np.array([0, nE - 1, nE, -1, 2 ** 31 + 5, 3], np.int64)
    ents, rels = fwd_ref.expand_ids(adj_e, adj_r, items, K, 2, nE)
    assert ents[0].ravel().tolist() == [0, nE - 1, nE - 1, 0, nE - 1, 3]
    # the definition, one element at a time
    for e in range(2):
        assert ents[e + 1].shape == (B, K ** (e + 1)) and rels[e].shape == (B, K ** (e + 1))
        for b in range(B):
            for j in range(K ** e):
                for k in range(K):
                    assert ents[e + 1][b, j * K + k] == adj_e[ents[e][b, j], k]
                    assert rels[e][b, j * K + k] == adj_r[ents[e][b, j], k]
    ents, rels = fwd_ref.expand_ids(adj_e, adj_r, items, K, 0, nE)
    assert len(ents) == 1 and rels == []


def test_precision_switch_reaches_every_function():
    rng = np.random.default_rng(8)
    src, W = rng.standard_normal((4, 8)), rng.standard_normal((8, 8))
    with fwd_ref.precision(np.float32):
        assert fwd_ref.linear([src], W, 8, rows=4)["out"].dtype == np.float32
        assert fwd_ref.agg(src, W, None, 2, child=rng.standard_normal((8, 8)), rel_score=rng.standard_normal(8))["out"].dtype == np.float32
        assert fwd_ref.ripple_attn(src, np.zeros((2, 3), int), np.zeros((2, 3), int), 1, w=W[0])["o"].dtype == np.float32
        assert fwd_ref.rel_score(src, rng.standard_normal(24)).dtype == np.float32
    assert fwd_ref.linear([src], W, 8, rows=4)["out"].dtype == np.float64
