"""Reference of the grouped ranking head (mvin_rank_head, training.Trainer.set_objective) -- TEST INFRASTRUCTURE.

A ranked batch has B = n_g * G rows, group-major: row g*G + j is slot j of group g; slot 0 is the positive, the other slots
are negatives of the same user; valid[g, j] in {0, 1} masks slots and slot 0 always counts.  V_g = valid slots, N_g = V_g \\ {0}.
  "softmax"  l_g = log sum_{j in V_g} exp(s[g,j]) - s[g,0]
  "bpr"      l_g = (1 / |N_g|) sum_{j in N_g} softplus(s[g,j] - s[g,0]), 0 for an empty N_g
The data term of the step is scale * sum_g l_g with scale = 1 / (n_g * world).  The regularisers of model.py:382-412 stay as
oracle/train_ref.py states them, over EVERY fed row, masked rows included.

``rank_head_ref`` evaluates the head in numpy at a chosen precision: float64 is the reference, float32 the straightforward
single-precision evaluation the GPU tests take as their yardstick.  ``ranked_loss_and_grads`` puts the head in place of the
cross-entropy term of oracle.train_ref.loss_from_params and back-propagates with autograd.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import train_ref

MODES = ("softmax", "bpr")


def valid_mask(valid, n_groups, G):
    """bool [n_groups, G]; None = all valid; slot 0 always counts."""
    val = np.ones((n_groups, G), dtype=bool) if valid is None else (np.asarray(valid).reshape(n_groups, G) != 0)
    val = val.copy()
    val[:, 0] = True
    return val


def pair_counts(scores, valid, G):
    """(c0, c1) of mvin_rank_head as Python ints from a score vector: c0 = sum over valid negatives of
    2 * [s < s_pos] + [s == s_pos], c1 = the number of valid negatives."""
    s = np.asarray(scores).reshape(-1, G)
    neg = valid_mask(valid, s.shape[0], G)
    neg[:, 0] = False
    s0 = s[:, :1]
    c0 = 2 * int(np.count_nonzero(neg & (s < s0))) + int(np.count_nonzero(neg & (s == s0)))
    return c0, int(np.count_nonzero(neg))


def rank_head_ref(x, valid, G, mode, dtype=np.float64):
    """``x``: the scores [B], or (user_o, item_emb) [B, D] each (the scores are then their row dot products).  Everything is
    computed in ``dtype``.  Returns a namespace, every gradient PER UNIT SCALE:
      scores [B], loss_groups [n_g], loss (their sum, accumulated in group order in ``dtype``), dscore [B],
      du / di [B, D] (None when scores were given), counts (c0, c1) from these scores."""
    if mode not in MODES:
        raise ValueError(mode)
    u = v = None
    if isinstance(x, tuple):
        u, v = (np.asarray(t, dtype=dtype) for t in x)
        s = (u * v).sum(axis=-1, dtype=dtype)
    else:
        s = np.asarray(x, dtype=dtype)
    s = s.reshape(-1, G)
    n_g = s.shape[0]
    val = valid_mask(valid, n_g, G)
    one, zero = dtype(1), dtype(0)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "softmax":
            sm = np.where(val, s, dtype(-np.inf))
            m = sm.max(axis=1, keepdims=True)
            e = np.where(val, np.exp(sm - m), zero).astype(dtype)
            Z = e.sum(axis=1, keepdims=True, dtype=dtype)
            ds = e / Z
            ds[:, 0] -= one
            ds = np.where(val, ds, zero).astype(dtype)
            loss_g = (np.log(Z[:, 0]) + (m[:, 0] - s[:, 0])).astype(dtype)
        else:
            neg = val.copy()
            neg[:, 0] = False
            d = s - s[:, :1]
            ex = np.exp(-np.abs(d))
            sig = (np.where(d >= 0, one, ex) / (one + ex)).astype(dtype)
            sp = (np.maximum(d, zero) + np.log1p(ex)).astype(dtype)
            cnt = np.maximum(neg.sum(axis=1), 1).astype(dtype)
            ds = (np.where(neg, sig, zero) / cnt[:, None]).astype(dtype)
            ds[:, 0] = -ds[:, 1:].sum(axis=1, dtype=dtype)
            loss_g = (np.where(neg, sp, zero).sum(axis=1, dtype=dtype) / cnt).astype(dtype)
    total = dtype(0)
    for l in loss_g:                     # plain accumulation in group order, in ``dtype``
        total = dtype(total + l)
    ds = ds.reshape(-1)
    du = di = None
    if u is not None:
        du, di = (ds[:, None] * v).astype(dtype), (ds[:, None] * u).astype(dtype)
    return SimpleNamespace(scores=s.reshape(-1), loss_groups=loss_g, loss=total, dscore=ds, du=du, di=di,
                           counts=pair_counts(s.reshape(-1), val, G))


def rank_head_torch(scores, valid, G, mode):
    """The group losses [n_g] as a differentiable torch expression (logsumexp / softplus) of a score vector [B]."""
    s = scores.view(-1, G)
    val = torch.from_numpy(valid_mask(None if valid is None else np.asarray(valid), s.shape[0], G))
    if mode == "softmax":
        return torch.logsumexp(s.masked_fill(~val, float("-inf")), dim=1) - s[:, 0]
    neg = val.clone()
    neg[:, 0] = False
    sp = torch.nn.functional.softplus(s - s[:, :1]) * neg.to(s.dtype)
    return sp.sum(dim=1) / neg.sum(dim=1).clamp(min=1).to(s.dtype)


def ranked_loss_and_grads(args, params, adj_entity, adj_relation, users, items, valid, mem_h, mem_r, mem_t, G, mode, world=1,
                          dtype=torch.float32):
    """The ranked step's loss and gradients: oracle.train_ref.loss_from_params gives ``out.scores`` and the l2 / l2agg pieces
    (computed over every fed row, masked rows included); the grouped head, mean over the n_g * world groups, takes the place of
    its cross-entropy term; autograd in ``dtype``.  Returns (loss float, grads dict of numpy arrays) like
    train_ref.loss_and_grads."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    B = len(np.asarray(items))
    if B % G:
        raise ValueError(f"{B} rows are not whole groups of {G}")
    _, pieces, out = train_ref.loss_from_params(args, p, adj_entity, adj_relation, users, items, np.zeros(B, dtype=np.float32),
                                                mem_h, mem_r, mem_t, dtype=dtype)
    head = rank_head_torch(out.scores, valid, G, mode).sum() / ((B // G) * world)
    loss = head + args.l2_weight * pieces["l2"] + args.l2_agg_weight * pieces["l2agg"]
    loss.backward()
    grads = {k: t.grad.numpy().copy() for k, t in p.items() if t.grad is not None}
    return float(loss.detach()), grads
