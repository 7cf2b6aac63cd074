"""Reference of the grouped ranking head WITH per-row logit offsets (mvin_rank_head_offset, Trainer.set_objective(offset=True))
and of the logQ offsets of an epoch (NegativeSampler.log_proposal, data_prep.rank_offsets) -- TEST INFRASTRUCTURE beside
tests/rank_loss_ref.py, which stays the reference of the head without offsets.

The loss of both modes is evaluated on z[g,j] = s[g,j] - offset[g,j] for every valid slot, slot 0 included:
  "softmax"  l_g = log sum_{j in V_g} exp(z[g,j]) - z[g,0]
  "bpr"      l_g = (1 / |N_g|) sum_{j in N_g} softplus(z[g,j] - z[g,0]), 0 for an empty N_g
dscore is dl/ds (dz/ds = 1), the scores reported and the pair counts are those of the RAW s, and the offset of an invalid slot
enters nothing (it is replaced by 0 before any arithmetic, whatever it holds).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

import rank_loss_ref as rl
from oracle import train_ref

MODES = rl.MODES


def clean_offset(offset, valid, n_groups, G, dtype):
    """[n_groups, G] in ``dtype``: ``offset`` (None: zeros) with 0 written into every invalid slot."""
    val = rl.valid_mask(valid, n_groups, G)
    if offset is None:
        return np.zeros((n_groups, G), dtype=dtype)
    c = np.asarray(offset, dtype=dtype).reshape(n_groups, G)
    return np.where(val, c, dtype(0)).astype(dtype)


def rank_head_offset_ref(x, valid, offset, G, mode, dtype=np.float64):
    """rank_loss_ref.rank_head_ref with logit offsets [B] (None: none): the same formulas, evaluated on z = s - offset in
    ``dtype``; ``scores`` and ``counts`` are those of the raw s.  Same namespace, every gradient per unit scale."""
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
    val = rl.valid_mask(valid, n_g, G)
    one, zero = dtype(1), dtype(0)
    z = (s - clean_offset(offset, valid, n_g, G, dtype)).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "softmax":
            zm = np.where(val, z, dtype(-np.inf))
            m = zm.max(axis=1, keepdims=True)
            e = np.where(val, np.exp(zm - m), zero).astype(dtype)
            Z = e.sum(axis=1, keepdims=True, dtype=dtype)
            ds = e / Z
            ds[:, 0] -= one
            ds = np.where(val, ds, zero).astype(dtype)
            loss_g = (np.log(Z[:, 0]) + (m[:, 0] - z[:, 0])).astype(dtype)
        else:
            neg = val.copy()
            neg[:, 0] = False
            d = z - z[:, :1]
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
                           counts=rl.pair_counts(s.reshape(-1), val, G))


def rank_head_offset_torch(scores, valid, offset, G, mode):
    """The group losses [n_g] as a differentiable torch expression of a score vector [B] and constant offsets [B] / None."""
    n_g = scores.numel() // G
    c = clean_offset(offset, valid, n_g, G, np.float64).reshape(-1)
    return rl.rank_head_torch(scores - torch.from_numpy(c).to(scores.dtype), valid, G, mode)


# --------------------------------------------------------------------------- the proposal and an epoch's offsets, restated
def _np(t):
    return np.asarray(t.cpu() if torch.is_tensor(t) else t)


def log_proposal_np(sampler):
    """NegativeSampler.log_proposal restated with plain loops: (p float64 [n_item], user_mass float64 [n_user], eligible
    counts int [n_user]).  p from ``alias_probabilities`` of the sampler's table (1 / n_item without one), 0 for masked items;
    the mass of a user sums p over the items outside the user's exclusion row, item by item."""
    from mvin_amd import data_prep
    n_item, n_user = sampler.n_item, sampler.n_user
    if sampler.alias is None:
        p = [1.0 / n_item] * n_item
        masked = [False] * n_item
    else:
        tab = _np(sampler.alias[0]).astype(np.int64) & 0xFFFFFFFF        # the device copy holds the words as int32
        p = data_prep.alias_probabilities(tab.astype(np.uint32)).tolist()
        words = [] if sampler.alias[1] is None else (_np(sampler.alias[1]).astype(np.int64) & 0xFFFFFFFF).tolist()
        masked = [bool(words and (words[i // 32] >> (i % 32)) & 1) for i in range(n_item)]
        p = [0.0 if masked[i] else p[i] for i in range(n_item)]
    ptr, ids = _np(sampler.excl[0]).tolist(), _np(sampler.excl[1]).tolist()
    mass, count = [], []
    for u in range(n_user):
        out = set(i for i in ids[ptr[u]:ptr[u + 1]] if 0 <= i < n_item)
        keep = [i for i in range(n_item) if i not in out and not masked[i]]
        mass.append(math.fsum(p[i] for i in keep))
        count.append(len(keep))
    return np.array(p), np.array(mass), np.array(count)


def rank_offsets_np(sampler, users, items, valid):
    """data_prep.rank_offsets restated: float32 [n, G]; slot 0 and invalid slots 0, a valid negative
    log(n_g * p_item / user_mass_u) evaluated in float64 and rounded once."""
    p, mass, _ = log_proposal_np(sampler)
    users, items, valid = _np(users), _np(items), _np(valid)
    n, G = items.shape
    out = np.zeros((n, G), dtype=np.float32)
    for g in range(n):
        negs = [j for j in range(1, G) if valid[g, j] != 0]
        for j in negs:
            out[g, j] = np.float32(math.log(len(negs)) + math.log(p[items[g, j]]) - math.log(mass[users[g]]))
    return out


def ranked_loss_and_grads(args, params, adj_entity, adj_relation, users, items, valid, offset, mem_h, mem_r, mem_t, G, mode,
                          world=1, dtype=torch.float32):
    """rank_loss_ref.ranked_loss_and_grads with logit offsets [B] (None: none): oracle.train_ref.loss_from_params gives
    ``out.scores`` and the l2 / l2agg pieces; the grouped head on scores - offset, mean over the n_g * world groups, takes the
    place of its cross-entropy term; autograd in ``dtype``.  Returns (loss float, grads dict of numpy arrays)."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    B = len(np.asarray(items))
    if B % G:
        raise ValueError(f"{B} rows are not whole groups of {G}")
    _, pieces, out = train_ref.loss_from_params(args, p, adj_entity, adj_relation, users, items, np.zeros(B, dtype=np.float32),
                                                mem_h, mem_r, mem_t, dtype=dtype)
    head = rank_head_offset_torch(out.scores, valid, offset, G, mode).sum() / ((B // G) * world)
    loss = head + args.l2_weight * pieces["l2"] + args.l2_agg_weight * pieces["l2agg"]
    loss.backward()
    grads = {k: t.grad.numpy().copy() for k, t in p.items() if t.grad is not None}
    return float(loss.detach()), grads
