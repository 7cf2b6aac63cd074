"""A plain reference for everything above key addressing in its folded forms (mvin_fold_tables -> mvin_score_l2_folded_fwd,
mvin_fold_tables_ex(aggregates = 0) -> mvin_score_l2_folded_gather_fwd, mvin_entity_aggregates -> mvin_gather_attn_l2_agg_fwd -> mvin_l2_tail_fwd):
the UNFOLDED formulas of include/mvin_hip.h (mvin_gather_attn_l2_fwd, then the tail of mvin_l2_tail_fwd) with plain torch indexing on the
PLAIN adjacency -- no projected table, no per-entity sum, no encoded slot word.  Nothing here is shared with the code under test."""
import torch


def clamp_ids(items, n_entity):
    """Item ids as the kernels read them: the low 32-bit word, unsigned, clamped to the table's last row."""
    return (items.long() & 0xFFFFFFFF).clamp(max=n_entity - 1)


def slot_weights(t, rel, dt):
    """Weights of the slots along the last axis: softmax of the relations' logits, or ones (the plain mean) without logits."""
    if t is None:
        return torch.ones(rel.shape, dtype=dt, device=rel.device)
    return torch.softmax(t.to(dt)[rel.long()], dim=-1)


def tail_reference(E, x, q, user_o, nagg0, nagg1, W0, b0, A0, a0, A1, a1, Wmix, bmix, dtype=torch.float64):
    """mvin_l2_tail_fwd's formulas for the (clamped) items x: -> item_emb [n, D], scores [n], sigmoid(scores) [n].  W0 = None (User_orient
    off): ev0 = E[x]; q and b0 are not used."""
    f = lambda t: t.to(dtype)                                 # noqa: E731
    z = lambda t: 0 if t is None else t.to(dtype)             # noqa: E731
    ev0 = f(E[x]) if W0 is None else (f(E[x]) + f(q)) @ f(W0) + z(b0)
    out0 = torch.relu((ev0 + f(nagg0)) @ f(A0) + z(a0))
    out2 = torch.relu((out0 + f(nagg1)) @ f(A1) + z(a1))
    item = torch.cat([ev0, out0, out2], dim=1) @ f(Wmix) + z(bmix)
    s = (f(user_o) * item).sum(1)
    return item, s, torch.sigmoid(s)


def fold_reference(E, adj_e, adj_r, items, t0, t1, q, user_o, W0, b0, W1, b1, W2, b2, A0, a0, A1, a1, Wmix, bmix, K, dtype=torch.float64):
    """-> nagg0, nagg1, item_emb, scores, sigmoid for the pairs (items[i], q[i], user_o[i]); E [n_entity, D], adj_e / adj_r [n_entity, K]
    the plain adjacency.  Biases that are None count as zero; t0 / t1 = None means slot weights of one (the plain mean, NOT a softmax of
    zeros); ids are clamped as unsigned words.  ``dtype`` = torch.float32 evaluates the same formulas op by op in fp32."""
    assert adj_e.shape[1] == K
    f = lambda t: t.to(dtype)                                 # noqa: E731
    z = lambda t: 0 if t is None else t.to(dtype)             # noqa: E731
    x = clamp_ids(items, E.shape[0])
    x1 = adj_e[x].long()                                      # [n, K]    children
    y = adj_e[x1].long()                                      # [n, K, K] grandchildren
    p = slot_weights(t0, adj_r[x1], dtype)                    # [n, K, K]
    c1 = f(q) @ f(W1) + z(b1)
    c2 = f(q) @ f(W2) + z(b2)
    self1 = f(E[x1]) @ f(W1) + c1[:, None, :]
    S = (p[..., None] * f(E[y])).sum(2)                       # [n, K, D]
    Z = self1 + (S @ f(W2) + p.sum(-1, keepdim=True) * c2[:, None, :]) / K
    out1 = torch.relu(Z @ f(A0) + z(a0))
    p0 = slot_weights(t0, adj_r[x], dtype)
    p1 = slot_weights(t1, adj_r[x], dtype)
    nagg0 = (p0[..., None] * self1).sum(1) / K
    nagg1 = (p1[..., None] * out1).sum(1) / K
    item, s, sg = tail_reference(E, x, q, user_o, nagg0, nagg1, W0, b0, A0, a0, A1, a1, Wmix, bmix, dtype)
    return nagg0, nagg1, item, s, sg


TAIL_BOUNDS = {"item_emb": (1e-5, 2e-6), "scores": (1e-5, 4e-6), "sigmoid": (1e-5, 1e-6), "nagg0": (1e-5, 2e-6), "nagg1": (1e-5, 2e-6)}


def compare(names, got, ref64, ref32, what, fails, hold_tail=True, stats=None, key=None, yard=None):
    """The project's rule for the folded form, per output: err_hip = max |got - float64| <= 4 err_f32 + 2e-6 with err_f32 = max |fp32
    evaluation of the same reference - float64|; and, where ``hold_tail``, the absolute bounds of the tail and aggregates tests against
    float64 (TAIL_BOUNDS: rtol, atol; ``hold_tail`` may be one flag per output).  ``yard``: err_f32 per output measured by the caller over
    a superset of these pairs.  Misses are appended to ``fails``; ``stats[(key, name)]`` keeps the worst
    [err_hip, err_f32, err_hip / (4 err_f32 + 2e-6), error / absolute bound]."""
    for i, (name, g, r64, r32) in enumerate(zip(names, got, ref64, ref32)):
        err = (g.double() - r64).abs()
        err_hip, err_f32 = float(err.max()), float((r32.double() - r64).abs().max())
        if yard is not None:                                  # err_f32 over a larger sample of the same reference (never a smaller one)
            err_f32 = max(err_f32, yard[i])
        hold = hold_tail[i] if isinstance(hold_tail, (list, tuple)) else hold_tail
        rel = err_hip / (4 * err_f32 + 2e-6)
        rtol, atol = TAIL_BOUNDS[name]
        tail = float((err / (rtol * r64.abs() + atol)).max())
        if stats is not None:
            s = stats.setdefault((key, name), [0.0, 0.0, 0.0, 0.0])
            s[:] = [max(a, b) for a, b in zip(s, (err_hip, err_f32, rel, tail))]
        if not rel <= 1.0:
            fails.append(f"{what} {name}: err_hip {err_hip:.3e} > 4 x err_f32 {err_f32:.3e} + 2e-6")
        if hold and not tail <= 1.0:
            fails.append(f"{what} {name}: {tail:.2f} x the absolute bound (rtol {rtol:g}, atol {atol:g}); err_hip {err_hip:.3e}, err_f32 {err_f32:.3e}")


def report(stats, key):
    for (k, name), s in stats.items():
        if k == key:
            print(f"MEASURED {k} {name}: err_hip {s[0]:.3e} err_f32 {s[1]:.3e} err/(4 err_f32 + 2e-6) {s[2]:.3f} err/absolute bound {s[3]:.3f}")


def fold_tables_reference(E, adj_e, adj_r, t0, W0, W1, W2, A0, Wmix, K, rows=None):
    """The float64 definitions of the tables of mvin_fold_tables for the entities ``rows`` (all of them when None):
    -> dict TA1, TA2, T0A, M0, H0, G, each [len(rows), D].  w(e)_k = the slot weights of entity e under t0, over K."""
    d = lambda t: t.double()                                  # noqa: E731
    n_entity, D = E.shape
    rows = torch.arange(n_entity, device=E.device) if rows is None else rows.long()
    y = adj_e[rows].long()                                    # [n, K]
    w = slot_weights(t0, adj_r[rows], torch.float64) / K
    Er, Ey = d(E[rows]), d(E[y])
    WA1, WA2, WA0 = d(W1) @ d(A0), d(W2) @ d(A0), d(W0) @ d(A0)
    TA1, TA2, T0A = Er @ WA1, Er @ WA2, Er @ WA0
    return {"TA1": TA1, "TA2": TA2, "T0A": T0A, "M0": Er @ d(W0) @ d(Wmix[:D]),
            "H0": T0A + (w[..., None] * (Ey @ WA1)).sum(1), "G": TA1 + (w[..., None] * (Ey @ WA2)).sum(1)}


def aggregates_reference(E, adj_e, adj_r, t0, W1, W2, A0, K, rows=None):
    """The float64 definitions of S0 | G of mvin_entity_aggregates over the projected tables, for the entities ``rows``."""
    d = lambda t: t.double()                                  # noqa: E731
    rows = torch.arange(E.shape[0], device=E.device) if rows is None else rows.long()
    y = adj_e[rows].long()
    w = slot_weights(t0, adj_r[rows], torch.float64) / K
    Er, Ey = d(E[rows]), d(E[y])
    return {"S0": (w[..., None] * (Ey @ d(W1))).sum(1), "G": Er @ d(W1) @ d(A0) + (w[..., None] * (Ey @ d(W2) @ d(A0))).sum(1)}
