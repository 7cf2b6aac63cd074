"""CPU: the float64 kernel references of tests/bwd_ref.py against torch.autograd (float64) on the forward formulas they
are the backward of (oracle/mirror_fp32.py, oracle/equations_fp64.py), at small random shapes.  A wrong reference would
bless a wrong kernel in tests/test_gpu_bwd_kernels.py; this module is what stands between."""
import numpy as np
import pytest
import torch

import bwd_ref
from oracle import train_ref

T64 = torch.float64


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=T64, requires_grad=grad)


def close(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-12 * max(1.0, float(np.abs(ref).max())), err_msg=what)


# ----------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("mode", ["dense1", "concat3_ids32", "sum2_ids64", "concat2_mixed"])
@pytest.mark.parametrize("nz,masked,pad", [(1, False, 0), (3, True, 5), (2, True, 0)])
def test_wgrad_is_the_gradient_of_the_staged_linear_layer(mode, nz, masked, pad):
    rng = np.random.default_rng(len(mode) * 100 + nz * 10 + pad)
    rows, Dsrc, Dout, ntab = 37, 8, 12, 9
    nsrc = {"dense1": 1, "concat3_ids32": 3, "sum2_ids64": 2, "concat2_mixed": 2}[mode]
    sum_sources = mode == "sum2_ids64"
    srcs, ids = [], []
    for s in range(nsrc):
        gathered = mode in ("concat3_ids32", "sum2_ids64") or (mode == "concat2_mixed" and s == 1)
        srcs.append(rng.standard_normal((ntab if gathered else rows, Dsrc)))
        ids.append(rng.integers(0, ntab, rows).astype(np.int64 if sum_sources else np.int32) if gathered else None)
    Din = Dsrc if sum_sources else nsrc * Dsrc
    ldy, ldm = Dout + pad, Dout + 2 * pad
    dy_zs, m_zs = rows * ldy + 3, rows * ldm + 1
    dY = rng.standard_normal(nz * dy_zs)
    W, b = rng.standard_normal((nz, Din, Dout)), rng.standard_normal((nz, Dout))
    # forward: out[z] = act(X W[z] + b[z]); L = sum_z sum(out[z] * G[z]) with G[z] the strided view of dY
    ts = [t64(s, True) for s in srcs]
    parts = [t[torch.as_tensor(i.astype(np.int64))] if i is not None else t for t, i in zip(ts, ids)]
    X = sum(parts[1:], parts[0]) if sum_sources else torch.cat(parts, dim=1)
    Wt, bt = t64(W, True), t64(b, True)
    L, masks = 0, np.zeros(nz * m_zs)
    for z in range(nz):
        pre = X @ Wt[z] + bt[z]
        out = torch.relu(pre) if masked else pre
        L = L + (out * t64(bwd_ref.strided(dY, z, dy_zs, rows, ldy, Dout))).sum()
        idx = z * m_zs + np.arange(rows)[:, None] * ldm + np.arange(Dout)[None, :]
        masks[idx] = out.detach().numpy()           # the mask is the forward OUTPUT (relu: > 0 where it passed)
    L.backward()
    dW, db = bwd_ref.wgrad(srcs, dY, Dout, ids=ids, sum_sources=sum_sources, mask=masks if masked else None, rows=rows,
                           nz=nz, ldy=ldy, dy_zstride=dy_zs, ldm=ldm, mask_zstride=m_zs)
    close(dW, Wt.grad.numpy(), "dW")
    close(db, bt.grad.numpy(), "db")
    # the magnitude bounds the value, and equals it on non-negative inputs
    mW, mb = bwd_ref.wgrad(srcs, dY, Dout, ids=ids, sum_sources=sum_sources, mask=masks if masked else None, rows=rows,
                           nz=nz, ldy=ldy, dy_zstride=dy_zs, ldm=ldm, mask_zstride=m_zs, magnitude=True)
    assert np.all(np.abs(dW) <= mW + 1e-12) and np.all(np.abs(db) <= mb + 1e-12)


# ----------------------------------------------------------------------------------------------- neighbor mix
def _agg_case(rng, T, K, D, nR, n_rows):
    return dict(dvec=rng.standard_normal((T, D)), table=rng.standard_normal((n_rows, D)),
                adj_e=rng.integers(0, n_rows, (n_rows, K)).astype(np.int32),
                adj_r=rng.integers(0, nR, (n_rows, K)).astype(np.int32), score=rng.standard_normal(nR))


@pytest.mark.parametrize("K,D,nR", [(3, 8, 4), (5, 12, 7), (8, 16, 2)])
@pytest.mark.parametrize("weights", ["probs", "rel_score", "mean"])
def test_agg_bwd_dense_form(K, D, nR, weights):
    rng = np.random.default_rng(K * 100 + D)
    T = 11
    c = _agg_case(rng, T, K, D, nR, 20)
    child, rel = rng.standard_normal((T * K, D)), rng.integers(0, nR, T * K).astype(np.int32)
    ct, st = t64(child, True), t64(c["score"], True)
    p = torch.softmax(st[torch.as_tensor(rel.astype(np.int64))].reshape(T, K), dim=-1) if weights != "mean" \
        else torch.ones((T, K), dtype=T64)
    agg = (p.unsqueeze(-1) * ct.reshape(T, K, D)).mean(dim=1)            # aggregators.py:141-144 / :148-152
    (agg * t64(c["dvec"])).sum().backward()
    kw = {"probs": p.detach().numpy()} if weights == "probs" else {}
    got = bwd_ref.agg_bwd(c["dvec"], K, nR, child=child, rel_ids=rel if weights != "mean" else None, **kw,
                          rel_score=None if weights != "rel_score" else c["score"])
    close(got["dchild"], ct.grad.numpy(), "dchild")
    if weights == "mean":
        assert got["dT"] is None
    else:
        close(got["dT"], st.grad.numpy(), "dT")


@pytest.mark.parametrize("K,D,nR", [(3, 8, 4), (5, 12, 7), (16, 32, 3)])
@pytest.mark.parametrize("form", ["gather_probs", "gather_mean", "by_entity"])
def test_agg_bwd_gather_and_by_entity_forms(K, D, nR, form):
    rng = np.random.default_rng(K * 100 + D + 1)
    n_rows = 23
    T = n_rows if form == "by_entity" else 14
    c = _agg_case(rng, T, K, D, nR, n_rows)
    node = None if form == "by_entity" else rng.integers(0, n_rows, T).astype(np.int32)
    if form == "by_entity":
        c["dvec"][rng.random(T) < 0.5] = 0.0                              # skipped rows contribute nothing anyway
    x = torch.arange(T) if node is None else torch.as_tensor(node.astype(np.int64))
    tt, st = t64(c["table"], True), t64(c["score"], True)
    ce, cr = torch.as_tensor(c["adj_e"].astype(np.int64))[x], torch.as_tensor(c["adj_r"].astype(np.int64))[x]
    p = torch.softmax(st[cr], dim=-1) if form != "gather_mean" else torch.ones((T, K), dtype=T64)
    agg = (p.unsqueeze(-1) * tt[ce]).mean(dim=1)
    (agg * t64(c["dvec"])).sum().backward()
    kw = dict(table=c["table"], adj_entity=c["adj_e"], node_ids=node)
    if form == "gather_probs":
        kw.update(probs=p.detach().numpy(), adj_relation=c["adj_r"])
    elif form == "by_entity":
        kw.update(rel_score=c["score"], adj_relation=c["adj_r"])
    got = bwd_ref.agg_bwd(c["dvec"], K, nR, **kw)
    close(got["dtable"], tt.grad.numpy(), "dtable")
    if form == "gather_mean":
        assert got["dT"] is None
    else:
        close(got["dT"], st.grad.numpy(), "dT")
    mag = bwd_ref.agg_bwd(c["dvec"], K, nR, magnitude=True, **kw)
    assert np.all(np.abs(got["dtable"]) <= mag["dtable"] + 1e-12)


def test_rel_score_bwd():
    rng = np.random.default_rng(5)
    nR, D = 7, 12
    rel, w, dT = rng.standard_normal((nR, D)), rng.standard_normal(3 * D), rng.standard_normal(nR)
    rt, wt = t64(rel, True), t64(w, True)
    ((rt @ wt[D:2 * D]) * t64(dT)).sum().backward()                       # t[r] = Rel[r] . urh_w[D:2D]
    drel, durh = bwd_ref.rel_score_bwd(rel, w, dT)
    close(drel, rt.grad.numpy())
    close(durh, wt.grad.numpy())


# ----------------------------------------------------------------------------------------------- key addressing
@pytest.mark.parametrize("P,has_set,item_share", [(0, True, False), (1, False, False), (1, True, True), (2, True, False),
                                                  (3, False, True), (2, True, True)])
@pytest.mark.parametrize("D,Nm,nR", [(8, 5, 3), (12, 3, 4), (16, 12, 2)])
def test_key_addressing_bwd(P, has_set, item_share, D, Nm, nR):
    rng = np.random.default_rng(P * 1000 + D * 10 + Nm + has_set)
    B, nE, l2 = 6, 17, 0.03
    E, Rk = rng.standard_normal((nE, D)), rng.standard_normal((nR, D, D)) * 0.3
    items = rng.integers(0, nE, B)
    w = rng.standard_normal(D) if has_set else None
    nh = max(1, P)
    mh = [rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(nh)]
    mr = [rng.integers(0, nR, (B, Nm)).astype(np.int32) for _ in range(P)]
    mt = [rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(P)]
    mh[0][2, :] = 4                                                        # all memories of a pair on one row
    nslot = P + (1 if has_set else 0)
    ldo = nslot * D + 4
    dout = rng.standard_normal(B * ldo)
    Et, wt, Rt = t64(E, True), (t64(w, True) if has_set else None), t64(Rk)
    if item_share:                                                         # V is a function of E[item]
        Vt = torch.einsum("bi,rij->brj", Et[torch.as_tensor(items)], Rt) if P else None
        if P:
            Vt.retain_grad()
    else:
        Vt = t64(rng.standard_normal((B, nR, D)), True) if P else None
    # forward in torch, as oracle/mirror_fp32.key_addressing states it (model.py:161-240) with V = E[item] . R
    L, slots = 0, []
    long = lambda a: torch.as_tensor(a.astype(np.int64))
    if has_set:
        h0 = Et[long(mh[0])]
        slots.append((torch.softmax(h0 @ wt, dim=-1).unsqueeze(-1) * h0).sum(dim=1))
    for hop in range(P):
        h, t = Et[long(mh[hop])], Et[long(mt[hop])]
        v = Vt[torch.arange(B).unsqueeze(1), long(mr[hop])]
        slots.append((torch.softmax((h * v).sum(-1), dim=-1).unsqueeze(-1) * t).sum(dim=1))
        L = L + l2 * ((h * h).sum() + (t * t).sum())
    out = torch.stack(slots, dim=1)
    Vn = Vt.detach().numpy() if P else None
    close(bwd_ref.key_addressing_fwd(E, Vn, w, mh, mr, mt, P, nR), out.detach().numpy(), "forward")
    G = t64(bwd_ref.strided(dout, 0, 0, B, ldo, nslot * D)).reshape(B, nslot, D)
    reg = float(L.detach()) if P else 0.0
    (L + (out * G).sum()).backward()
    got = bwd_ref.key_addressing_bwd(E, Vn, w, mh, mr, mt, P, dout, ldo, nR, l2,
                                     relation_kge=Rk if item_share and P else None, items=items if item_share and P else None)
    close(got["dE"], Et.grad.numpy(), "dE")
    if P:
        close(got["dV"], Vt.grad.numpy(), "dV")
        assert abs(got["reg"] - reg) <= 1e-12 * abs(reg)
    else:
        assert got["dV"] is None and got["reg"] == 0.0
    if has_set:
        close(got["dw"], wt.grad.numpy(), "dw")
    else:
        assert got["dw"] is None
    mag = bwd_ref.key_addressing_bwd(E, Vn, w, mh, mr, mt, P, dout, ldo, nR, l2, magnitude=True,
                                     relation_kge=Rk if item_share and P else None, items=items if item_share and P else None)
    assert np.all(np.abs(got["dE"]) <= mag["dE"] + 1e-12)


# ----------------------------------------------------------------------------------------------- small kernels
@pytest.mark.parametrize("idt", [np.int32, np.int64])
def test_scatter_add_rows_is_the_backward_of_a_row_lookup(idt):
    rng = np.random.default_rng(8)
    n, rows, D, alpha = 9, 40, 8, -0.75
    ids, x = rng.integers(0, n, rows).astype(idt), rng.standard_normal((rows, D))
    tab = t64(rng.standard_normal((n, D)), True)
    (alpha * tab[torch.as_tensor(ids.astype(np.int64))] * t64(x)).sum().backward()
    close(bwd_ref.scatter_add_rows(n, ids, x, alpha), tab.grad.numpy())


def test_count_ids():
    ids = np.array([0, 3, 3, -1, 4, 5, 0, 0, 2 ** 20, -7], np.int32)
    np.testing.assert_array_equal(bwd_ref.count_ids(ids, 5), [3, 0, 0, 2, 1])
    np.testing.assert_array_equal(bwd_ref.count_ids(ids, 1), [3])
    # the gradient of sum_i w[ids[i]]: one per occurrence
    wt = t64(np.zeros(6), True)
    wt[torch.as_tensor(ids[(ids >= 0) & (ids < 6)].astype(np.int64))].sum().backward()
    np.testing.assert_array_equal(bwd_ref.count_ids(ids, 6), wt.grad.numpy())


def test_eltwise_modes():
    rng = np.random.default_rng(9)
    rows, D, N = 12, 8, 3
    n = rows * D
    x, y, z = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    # 0: gradient accumulation y <- alpha x + beta y: the gradient of sum(p * (alpha x + beta y)) with respect to p
    pt = t64(np.ones(n), True)
    (pt * (0.5 * t64(x) - 2.0 * t64(y))).sum().backward()
    close(bwd_ref.eltwise(0, x, y, alpha=0.5, beta=-2.0)["y"], pt.grad.numpy())
    close(bwd_ref.eltwise(0, x, np.full(n, np.nan), alpha=0.5, beta=0.0)["y"], 0.5 * x)   # beta = 0: y is not read
    # 1: mean sigmoid cross entropy (model.py:379-380) and its gradient with respect to the logits
    lab = (rng.random(n) < 0.5).astype(np.float64)
    st = t64(x * 3, True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(st, t64(lab), reduction="mean")
    loss.backward()
    r = bwd_ref.eltwise(1, x * 3, z=lab, alpha=1.0 / n, beta=1.0 / n)
    close(r["y"], st.grad.numpy())
    assert abs(r["accum"] - float(loss.detach())) < 1e-12
    # 2: relu backward through the forward OUTPUT
    pre = t64(z, True)
    (torch.relu(pre) * t64(x)).sum().backward()
    close(bwd_ref.eltwise(2, x, z=np.maximum(z, 0))["y"], pre.grad.numpy())
    # 3: alpha sum x^2 as torch states it; its autograd gradient 2 alpha x is mode 0 with that factor
    xt = t64(x, True)
    sq = 0.25 * (xt * xt).sum()
    sq.backward()
    assert abs(bwd_ref.eltwise(3, x, alpha=0.25)["accum"] - float(sq.detach())) < 1e-12
    close(bwd_ref.eltwise(0, x, alpha=2 * 0.25)["y"], xt.grad.numpy())
    # 4: one Adam step == train_ref.AdamRef in float64 at t = 1 ... 3
    opt = train_ref.AdamRef({"p": x}, lr=0.01, dtype=np.float64)
    p, m, v = x.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 4):
        g = rng.standard_normal(n)
        ref = opt.step({"p": p.copy()}, {"p": g})["p"]
        lr_t = 0.01 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        r = bwd_ref.eltwise(4, p, g, m, v, alpha=lr_t, beta1=0.9, beta2=0.999, eps=1e-8)
        p, m, v = r["x"], r["z"], r["w"]
        close(p, ref), close(m, opt.m["p"]), close(v, opt.v["p"])
    X, zr = x.reshape(rows, D), rng.standard_normal(rows)
    # 5: the backward of a per-row scale out[r, :] = alpha z[r] in[r, :] with upstream gradient x, accumulated onto beta y
    it = t64(rng.standard_normal((rows, D)), True)
    (2.0 * t64(zr).unsqueeze(1) * it * t64(X)).sum().backward()
    close(bwd_ref.eltwise(5, x, y, zr, alpha=2.0, beta=0.0, D=D)["y"], it.grad.numpy().ravel())
    close(bwd_ref.eltwise(5, x, y, zr, alpha=2.0, beta=0.5, D=D)["y"], 0.5 * y + it.grad.numpy().ravel())
    # 6: the backward of a broadcast out[g N + q, :] = alpha in[g, :] over the N rows of a group, upstream gradient x
    gt = t64(rng.standard_normal((rows // N, D)), True)
    (-1.5 * gt.unsqueeze(1).expand(rows // N, N, D) * t64(X).reshape(rows // N, N, D)).sum().backward()
    close(bwd_ref.eltwise(6, x, alpha=-1.5, D=D, N=N)["y"], gt.grad.numpy().ravel())
    # 7: the row-weighted squared norm as torch states it; its autograd gradient 2 alpha z[r] x[r, :] is mode 5
    xt = t64(X, True)
    wsq = 0.5 * (t64(zr) * (xt * xt).sum(dim=1)).sum()
    wsq.backward()
    assert abs(bwd_ref.eltwise(7, x, z=zr, alpha=0.5, D=D)["accum"] - float(wsq.detach())) < 1e-12
    close(bwd_ref.eltwise(5, x, None, zr, alpha=2 * 0.5, D=D)["y"], xt.grad.numpy().ravel())
    ids = rng.integers(0, rows, 30).astype(np.int32)
    tab = t64(X, True)
    sq = 0.5 * (tab[torch.as_tensor(ids.astype(np.int64))] ** 2).sum()
    assert abs(bwd_ref.eltwise(8, x, z=ids, alpha=0.5, D=D)["accum"] - float(sq)) < 1e-12


@pytest.mark.parametrize("apply_adam", [False, True])
def test_l2_adam_over_a_segment_table(apply_adam):
    rng = np.random.default_rng(10)
    shapes, l2s = [(5,), (3, 4), (1,), (7,), (2, 8)], [0.0, 1e-2, 0.5, 0.0, 1e-3]
    xs = [rng.standard_normal(s) for s in shapes]
    total = sum(a.size for a in xs)
    g0 = rng.standard_normal(total)
    ts = [t64(a, True) for a in xs]
    L = sum(c / 2 * (t * t).sum() for t, c in zip(ts, l2s))               # tf.nn.l2_loss terms, model.py:387-412
    L.backward()
    gref = g0 + np.concatenate([t.grad.numpy().ravel() for t in ts])
    m0, v0 = rng.standard_normal(total) * 0.1, rng.random(total) * 0.1
    r = bwd_ref.l2_adam(xs, l2s, g0, m0, v0, apply_adam=apply_adam, lr_t=0.02, beta1=0.9, beta2=0.999, eps=1e-8)
    close(r["g"], gref)
    assert abs(r["loss"] - float(L)) < 1e-12
    if not apply_adam:
        for a, b in zip(r["xs"], xs):
            np.testing.assert_array_equal(a, b)
        return
    m = 0.9 * m0 + 0.1 * gref
    v = 0.999 * v0 + 0.001 * gref ** 2
    close(r["m"], m), close(r["v"], v)
    flat = np.concatenate([a.ravel() for a in xs]) - 0.02 * m / (np.sqrt(v) + 1e-8)
    close(np.concatenate([a.ravel() for a in r["xs"]]), flat)
    # and against train_ref.AdamRef (float64) from zero moments: its first step
    opt = train_ref.AdamRef({str(i): a for i, a in enumerate(xs)}, lr=0.01, dtype=np.float64)
    offs = np.cumsum([0] + [a.size for a in xs])
    ref = opt.step({str(i): a.astype(np.float64) for i, a in enumerate(xs)},
                   {str(i): gref[offs[i]:offs[i + 1]].reshape(a.shape) for i, a in enumerate(xs)})
    r = bwd_ref.l2_adam(xs, l2s, g0, np.zeros(total), np.zeros(total), apply_adam=True,
                        lr_t=0.01 * np.sqrt(1 - 0.999) / (1 - 0.9))
    for i, a in enumerate(r["xs"]):
        close(a, ref[str(i)])


# ----------------------------------------------------------------------------------------------- against the mirror itself
def test_agg_and_rel_score_backward_chain_against_the_mirrors_own_aggregator():
    """oracle/mirror_fp32.mix_neighbor_vectors_urh (aggregators.py:118-146) in float64: its logits are
    [user, relation, self] . urh_w, of which only the relation part t[r] = Rel[r] . urh_w[D:2D] varies over the
    neighbours, so agg_bwd on softmax(t[rel]) followed by rel_score_bwd must give autograd's gradients of the children,
    the relation table and the middle third of urh_w."""
    from oracle import mirror_fp32
    rng = np.random.default_rng(21)
    B, N, K, D, nR = 3, 4, 5, 8, 6
    rel_ids = rng.integers(0, nR, (B, N, K))
    child, Rel, urh = t64(rng.standard_normal((B, N, K, D)), True), t64(rng.standard_normal((nR, D)), True), \
        t64(rng.standard_normal((3 * D, 1)), True)
    self_v, user, dvec = t64(rng.standard_normal((B, N, D))), t64(rng.standard_normal((B, D))), rng.standard_normal((B * N, D))
    agg, probs = mirror_fp32.mix_neighbor_vectors_urh(self_v, user, child, Rel[torch.as_tensor(rel_ids)], urh, B, D)
    (agg.reshape(B * N, D) * t64(dvec)).sum().backward()
    score = Rel.detach().numpy() @ urh.detach().numpy()[D:2 * D, 0]
    got = bwd_ref.agg_bwd(dvec, K, nR, child=child.detach().numpy().reshape(-1, D), rel_ids=rel_ids.ravel(), rel_score=score)
    close(bwd_ref.softmax(score[rel_ids]).reshape(B, N, K), probs.detach().numpy(), "probs")
    close(got["dchild"], child.grad.numpy().reshape(-1, D), "dchild")
    drel, durh = bwd_ref.rel_score_bwd(Rel.detach().numpy(), urh.detach().numpy(), got["dT"])
    close(drel, Rel.grad.numpy(), "drel")
    close(durh[D:2 * D], urh.grad.numpy()[D:2 * D, 0], "durh")
    assert not np.any(durh[:D]) and not np.any(durh[2 * D:])
    # the user and self thirds of urh_w get no gradient from the mix: their logit terms are constant over k
    assert np.abs(urh.grad.numpy()[:D]).max() < 1e-12 and np.abs(urh.grad.numpy()[2 * D:]).max() < 1e-12


@pytest.mark.parametrize("P,ps_o_ft", [(2, True), (1, True), (2, False)])
def test_key_addressing_forward_is_the_mirrors(P, ps_o_ft):
    """bwd_ref.key_addressing_fwd slot by slot against oracle/mirror_fp32.key_addressing (model.py:161-240) in float64,
    with V[b, r, :] = E[item_b] . R_KGE[r], w = the entity half of h_emb_item_mlp_matrix and a user MLP that picks one
    slot of o_cat at a time."""
    from mvin_amd.config import make_args
    from oracle import mirror_fp32
    rng = np.random.default_rng(22 + P)
    B, D, Nm, nE, nR, nU = 5, 8, 6, 30, 4, 3
    args = make_args(dim=D, p_hop=P, n_memory=Nm, batch_size=B, PS_O_ft=int(ps_o_ft))
    nslot = P + (1 if ps_o_ft else 0)
    p = {"entity_emb_matrix": rng.standard_normal((nE, D)), "relation_emb_KGE_matrix": rng.standard_normal((nR, D, D)) * 0.3,
         "user_emb_matrix": rng.standard_normal((nU, D)), "h_emb_item_mlp_matrix": rng.standard_normal((2 * D, 1)),
         "h_emb_item_mlp_bias": rng.standard_normal(1), "user_mlp_bias": np.zeros(D)}
    users, items = rng.integers(0, nU, B), rng.integers(0, nE, B)
    mh = [rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(P)]
    mr = [rng.integers(0, nR, (B, Nm)).astype(np.int32) for _ in range(P)]
    mt = [rng.integers(0, nE, (B, Nm)).astype(np.int32) for _ in range(P)]
    V = np.einsum("bi,rij->brj", p["entity_emb_matrix"][items], p["relation_emb_KGE_matrix"])
    w = p["h_emb_item_mlp_matrix"][:D, 0] if ps_o_ft else None
    mine = bwd_ref.key_addressing_fwd(p["entity_emb_matrix"], V, w, mh, mr, mt, P, nR)
    assert mine.shape == (B, nslot, D)
    for s in range(nslot):
        pick = np.zeros((nslot * D, D))
        pick[s * D:(s + 1) * D] = np.eye(D)
        pt = {k: t64(v) for k, v in dict(p, user_mlp_matrix=pick).items()}
        user_o, _ = mirror_fp32.key_addressing(args, pt, torch.as_tensor(users), torch.as_tensor(items),
                                               [torch.as_tensor(m) for m in mh], [torch.as_tensor(m) for m in mr],
                                               [torch.as_tensor(m) for m in mt])
        close(mine[:, s], user_o.numpy(), f"slot {s}")
