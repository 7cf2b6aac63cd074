"""Host oracles of the matrix-factorisation feature (mvin_amd/mf.py; include/mvin_hip.h states the rules restated here).

  head64            mvin_mf_head in float64, straightforwardly: scores, loss, regulariser, dscore, du, di, counts.
  grad_rows32       the BIT rule of du / di in numpy float32, from a given (the device's own) dscore.
  adam_rows32       the BIT rule of mvin_sparse_adam_rows in numpy float32: stable run order, left-to-right sums, every
                    operation rounded on its own.
  lr_t32            the bias-corrected step size as float32 (training.Trainer.lr_t's rule).
  OracleTrainer     float64 lazy and dense Adam on float64 tables.
  planted, train_oracle, auc   the learning condition: planted low-rank data, the float64 restatement of train_mf's "bce"
                    epochs (same initial tables, same permutations), and a tie-aware AUC.
Own code: numpy only.
"""
import numpy as np

SOFTMAX, BPR, BCE = "softmax", "bpr", "bce"


def clamp(ids, n):
    return np.clip(np.asarray(ids, dtype=np.int64), 0, n - 1)


def effective_valid(valid, B, G, mode):
    """bool [B]: slot 0 of a ranking group is valid whatever ``valid`` says; in BCE mode (G = 1) ``valid`` masks any row."""
    val = np.ones(B, dtype=bool) if valid is None else (np.asarray(valid).reshape(-1) != 0)
    val = val.copy()
    if mode != BCE:
        val[::G] = True
    return val


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def head64(U, V, users, items, mode, scale, reg, G, valid=None, labels=None, dtype=np.float64):
    """dict of float64 results: scores [B], dscore [B] (scale included), du / di [B, D], loss (scale included), reg_loss,
    counts (2 ints).  U / V are taken as they are (float32 tables are widened exactly).  ``dtype=np.float32``: the same
    formulas with every array in float32 -- a plain restatement for tolerance yardsticks, not a bit rule."""
    U = np.asarray(U, dtype=dtype)
    V = np.asarray(V, dtype=dtype)
    items = np.asarray(items).reshape(-1)
    B, D = items.shape[0], U.shape[1]
    ug = U[clamp(users, U.shape[0])]
    ur = np.repeat(ug, G, axis=0)
    vr = V[clamp(items, V.shape[0])]
    s = (ur * vr).sum(axis=1)
    val = effective_valid(valid, B, G, mode)
    ds = np.zeros(B, dtype=dtype)
    loss, c0, c1 = 0.0, 0, 0
    if mode == BCE:
        y = np.where(val, np.asarray(labels, dtype=dtype).reshape(-1), dtype(0))     # a masked label is never looked at
        l = np.maximum(s, 0.0) - s * y + np.log1p(np.exp(-np.abs(s)))
        loss = float(l[val].sum())
        ds[val] = (_sigmoid(s) - y)[val]
    else:
        S, W = s.reshape(-1, G), val.reshape(-1, G)
        dS = ds.reshape(-1, G)
        for g in range(S.shape[0]):
            w = W[g]
            if mode == SOFTMAX:
                z = S[g][w]
                m = z.max()
                e = np.exp(z - m)
                loss += float(np.log(e.sum()) + m - S[g, 0])
                p = e / e.sum()
                p[0] -= 1.0
                dS[g][w] = p
            else:
                neg = w.copy()
                neg[0] = False
                n = int(neg.sum())
                if n:
                    x = S[g][neg] - S[g, 0]
                    loss += float(_softplus(x).sum() / n)
                    sg = _sigmoid(x) / n
                    dS[g][neg] = sg
                    dS[g, 0] = -sg.sum()
            neg = w.copy()
            neg[0] = False
            c0 += int(2 * (S[g][neg] < S[g, 0]).sum() + (S[g][neg] == S[g, 0]).sum())
            c1 += int(neg.sum())
    ds *= dtype(scale)
    reg = dtype(reg)
    first = np.zeros(B, dtype=bool)
    first[::G] = True
    di = np.where(val[:, None], ds[:, None] * ur + reg * vr, dtype(0))
    du = np.where(val[:, None], ds[:, None] * vr + reg * np.where(first[:, None], ur, dtype(0)), dtype(0))
    reg_loss = 0.5 * float(reg) * float((ur[val & first] ** 2).sum() + (vr[val] ** 2).sum())
    return dict(scores=s, dscore=ds, du=du, di=di, loss=scale * loss, reg_loss=reg_loss, counts=(c0, c1), valid=val)


def grad_rows32(U, V, users, items, dscore, reg, G, val):
    """(du, di) float32 [B, D] by the bit rule: di = add(mul(ds, u), mul(reg, v)); du = mul(ds, v), plus mul(reg, u) on slot 0;
    with reg == 0 the single products alone (no +0 is added); a masked row is +0 when reg != 0 and the product with its
    dscore of 0 otherwise.  ``val``: ``effective_valid``."""
    U, V = np.asarray(U, dtype=np.float32), np.asarray(V, dtype=np.float32)
    items = np.asarray(items).reshape(-1)
    ur = np.repeat(U[clamp(users, U.shape[0])], G, axis=0)
    vr = V[clamp(items, V.shape[0])]
    ds = np.asarray(dscore, dtype=np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        du, di = ds * vr, ds * ur
        if reg != 0:
            r = np.float32(reg)
            di = di + r * vr
            first = np.zeros(items.shape[0], dtype=bool)
            first[::G] = True
            du = np.where(first[:, None], du + r * ur, du)
            du = np.where(val[:, None], du, np.float32(0))
            di = np.where(val[:, None], di, np.float32(0))
    return du.astype(np.float32), di.astype(np.float32)


def lr_t32(lr, b1, b2, t):
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    return np.float32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def adam_rows32(x, m, v, keys, grads, valid, lr_t, b1, b2, eps, order=None):
    """mvin_sparse_adam_rows on float32 numpy arrays, IN PLACE.  Returns (rows updated, entries dropped)."""
    assert x.dtype == m.dtype == v.dtype == grads.dtype == np.float32
    keys = np.asarray(keys, dtype=np.int64)
    n, n_rows = keys.shape[0], x.shape[0]
    order = np.argsort(keys, kind="stable") if order is None else np.asarray(order, dtype=np.int64)
    lr_t, b1, b2, eps = np.float32(lr_t), np.float32(b1), np.float32(b2), np.float32(eps)
    c1, c2 = np.float32(1) - b1, np.float32(1) - b2
    kept = [int(o) for o in order if 0 <= o < n]
    dropped = len(order) - len(kept)
    runs, cur = [], None
    for o in kept:
        k = int(keys[o])
        bad = not 0 <= k < n_rows
        dropped += bad
        if cur is None or cur[0] != k:             # a run of an out-of-range key does nothing, but it separates runs
            cur = [k, []]
            if not bad:
                runs.append(cur)
        if not bad:
            cur[1].append(o)
    updated = 0
    with np.errstate(all="ignore"):
        for k, idx in runs:
            use = [o for o in idx if valid is None or valid[o] != 0]
            if not use:
                continue
            g = grads[use[0]].copy()
            for o in use[1:]:
                g = g + grads[o]
            m[k] = b1 * m[k] + c1 * g
            v[k] = b2 * v[k] + c2 * (g * g)
            x[k] = x[k] - lr_t * (m[k] / (np.sqrt(v[k]) + eps))
            updated += 1
    return updated, dropped


class OracleTrainer(object):
    """float64 Adam on float64 tables with head64's gradients.  ``adam`` "lazy": only the rows a batch's valid entries name
    move, and only their moments decay; "dense": TF1's -- every row of both tables takes the step."""

    def __init__(self, U, V, lr, reg=0.0, objective=BCE, group_size=1, adam="lazy", betas=(0.9, 0.999), eps=1e-8, f32_betas=True):
        self.U, self.V = np.array(U, dtype=np.float64), np.array(V, dtype=np.float64)
        self.lr, self.reg, self.mode, self.G, self.adam = lr, reg, objective, group_size, adam
        self.b1, self.b2 = (float(np.float32(betas[0])), float(np.float32(betas[1]))) if f32_betas else betas
        self.eps, self.t = float(np.float32(eps)) if f32_betas else eps, 0
        self.mu, self.vu = np.zeros_like(self.U), np.zeros_like(self.U)
        self.mi, self.vi = np.zeros_like(self.V), np.zeros_like(self.V)

    def _apply(self, x, m, v, keys, grads, val, lr_t):
        g = np.zeros_like(x)
        np.add.at(g, keys[val], grads[val])
        rows = np.unique(keys[val]) if self.adam == "lazy" else np.arange(x.shape[0])
        m[rows] = self.b1 * m[rows] + (1.0 - self.b1) * g[rows]
        v[rows] = self.b2 * v[rows] + (1.0 - self.b2) * g[rows] ** 2
        x[rows] -= lr_t * m[rows] / (np.sqrt(v[rows]) + self.eps)

    def step(self, users, items, valid=None, labels=None):
        items = np.asarray(items).reshape(-1)
        n_groups = np.asarray(users).shape[0]
        h = head64(self.U, self.V, users, items, self.mode, 1.0 / n_groups, self.reg, self.G, valid, labels)
        self.t += 1
        lr_t = float(lr_t32(self.lr, self.b1, self.b2, self.t))
        ukeys = np.repeat(clamp(users, self.U.shape[0]), self.G)
        self._apply(self.U, self.mu, self.vu, ukeys, h["du"], h["valid"], lr_t)
        self._apply(self.V, self.mi, self.vi, clamp(items, self.V.shape[0]), h["di"], h["valid"], lr_t)
        return h


# ---------------------------------------------------------------------------- the learning condition
def xavier64(n_user, n_item, dim, seed):
    """mf.xavier_tables restated: uniform(-a, a), a = sqrt(6 / (rows + dim)), U then V from default_rng(seed), as float32."""
    rng = np.random.default_rng(int(seed))
    out = []
    for rows in (n_user, n_item):
        a = np.sqrt(6.0 / (rows + dim))
        out.append(rng.uniform(-a, a, size=(rows, dim)).astype(np.float32))
    return out


def planted(seed, n_user=200, n_item=300, rank=4, per_user=40, train_share=0.8):
    """(train, test) int64 rows (user, item, label): rank-4 Gaussian factors, ``per_user`` distinct items drawn per user,
    label = [planted score > 0], split 80 / 20 by a seeded permutation of the rows."""
    rng = np.random.default_rng(1000 + seed)
    P, Q = rng.normal(size=(n_user, rank)), rng.normal(size=(n_item, rank))
    rows = []
    for u in range(n_user):
        it = rng.choice(n_item, size=per_user, replace=False)
        rows.append(np.stack([np.full(per_user, u), it, (P[u] @ Q[it].T > 0).astype(np.int64)], axis=1))
    rows = np.concatenate(rows).astype(np.int64)
    rows = rows[rng.permutation(rows.shape[0])]
    cut = int(train_share * rows.shape[0])
    return rows[:cut], rows[cut:]


def auc(scores, labels):
    """Tie-aware AUC (mean rank of the positives)."""
    scores, labels = np.asarray(scores, dtype=np.float64), np.asarray(labels)
    order = np.argsort(scores, kind="stable")
    s = scores[order]
    ranks = np.empty(len(s))
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    pos = labels == 1
    n1, n0 = int(pos.sum()), int((~pos).sum())
    return float((ranks[pos].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def train_oracle(train, n_user, n_item, dim, lr, reg, epochs, batch_size, seed, adam="lazy"):
    """train_mf's "bce" run in float64: the same initial tables, the same per-epoch permutations, the same batches."""
    U, V = xavier64(n_user, n_item, dim, seed)
    tr = OracleTrainer(U, V, lr, reg=reg, objective=BCE, group_size=1, adam=adam)
    for epoch in range(epochs):
        perm = np.random.default_rng([int(seed), epoch]).permutation(train.shape[0])
        for s0 in range(0, train.shape[0], batch_size):
            b = train[perm[s0:s0 + batch_size]]
            tr.step(b[:, 0], b[:, 1], labels=b[:, 2].astype(np.float64))
    return tr


def held_out_auc(tr, test):
    s = (tr.U[test[:, 0]] * tr.V[test[:, 1]]).sum(axis=1)
    return auc(s, test[:, 2])
