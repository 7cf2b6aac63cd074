"""Matrix factorisation (MF): the simplest baseline of the paper's tables (the reference's KGAT/BPRMF.py) and a learned
retrieval tower for the serving path.  score(u, i) = <U[u], V[i]> -- the quantity ops.mips_topk ranks.

    model, records = train_mf(train_data, n_user, n_item, lr=0.02, reg=1e-4, epochs=20, batch_size=512)
    mf = MFFeeder(model)
    compare_ctr([mvin_feeder, mf], test_data)                        # is MVIN significantly better than MF on this split?
    mvin_feeder.recommend_two_stage(users, k, n_cand, items, retriever=mf)
    retrieval_eval(mvin_feeder, ..., retriever=mf)                   # does the tower keep more of MVIN's top-k than the proxy?

A training step is the head (ops.mf_head: scores, loss, dscore and the gradient rows in one launch, rows read by id from the
tables) and an optimiser.  ``adam="lazy"`` (the default): two ops.sparse_adam_rows calls, which sum duplicate rows in one fixed
order -- a whole run is reproducible bit for bit, and rows a batch does not touch keep their moments (the SparseAdam
convention).  ``adam="dense"``: ops.scatter_add_rows into dense gradient buffers and ops.l2_adam_multi over both tables -- TF1's
semantics (every row decays at every step), the faithful form of the reference's baseline; its bits depend on atomic order and
its cost on the catalogue, not the batch.

Assumed: f32 tables, one GPU, dim a multiple of 4 in 4..128.  Out of scope: bias terms, bf16 tables, logQ offsets and hard
negatives for MF, hipGraph capture of the step.
"""
import types

import numpy as np
import torch

from . import ops
from .harness import DeviceFeeder, _dev_ids

OBJECTIVES = ("bce", "bpr", "softmax")


def xavier_tables(n_user, n_item, dim, seed=0):
    """(U float32 [n_user, dim], V float32 [n_item, dim]) on the host: Xavier-uniform, limit sqrt(6 / (rows + dim)), drawn in
    float64 from ``np.random.default_rng(seed)`` -- U first, then V -- and rounded once."""
    rng = np.random.default_rng(int(seed))
    out = []
    for rows in (int(n_user), int(n_item)):
        a = np.sqrt(6.0 / (rows + int(dim)))
        out.append(rng.uniform(-a, a, size=(rows, int(dim))).astype(np.float32))
    return out[0], out[1]


class MFModel(object):
    """The two tables.  ``entity_emb_matrix`` IS the item table V, so every retrieval method a feeder inherits (retrieve,
    similar_items, diversify_lists) finds its item rows where it looks for them."""

    def __init__(self, n_user, n_item, dim, seed=0, device="cuda"):
        n_user, n_item, dim = int(n_user), int(n_item), int(dim)
        if n_user < 1 or n_item < 1:
            raise ValueError(f"MFModel: n_user={n_user}, n_item={n_item}: both at least 1")
        if dim < 4 or dim > 128 or dim % 4:
            raise ValueError(f"MFModel: dim={dim}: a multiple of 4 in 4..128 (the kernels read rows in 16-byte chunks)")
        self.n_user, self.n_item, self.dim = n_user, n_item, dim
        self.device = torch.device(device)
        U, V = xavier_tables(n_user, n_item, dim, seed)
        self.user_emb_matrix = torch.from_numpy(U).to(self.device)
        self.entity_emb_matrix = torch.from_numpy(V).to(self.device)

    @property
    def item_emb_matrix(self):
        return self.entity_emb_matrix

    def forward_users(self, u, it, uts=None, distinct_users=None, **_):
        """Logits and their sigmoid of the pairs (u[i], it[i]) in ONE mvin_mf_scores launch; ``uts`` and ``distinct_users``
        are taken for the signature a feeder calls and not used (MF has no ripple sets)."""
        z, p = ops.mf_scores(self.user_emb_matrix, self.entity_emb_matrix, u.reshape(-1).contiguous(), it.reshape(-1).contiguous())
        return types.SimpleNamespace(scores=z, scores_normalized=p)


class MFTrainer(object):
    """Adam on an ``MFModel``.  ``objective`` "bce" (rows with labels; BPRMF.py's own), "bpr" or "softmax" (groups of
    ``group_size`` = 1 + negatives, slot 0 the positive: data_prep.rank_groups).  ``adam`` "lazy" or "dense" (module docstring).
    ``reg``: the coefficient c of (c / 2) * sum of squares over the batch's rows, every occurrence counted."""

    def __init__(self, model, lr, reg=0.0, objective="bce", group_size=None, adam="lazy", betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(model, MFModel):
            raise ValueError(f"MFTrainer: model must be an MFModel, got {type(model).__name__}")
        if objective not in OBJECTIVES:
            raise ValueError(f"MFTrainer: objective={objective!r}: expected one of {OBJECTIVES}")
        if adam not in ("lazy", "dense"):
            raise ValueError(f"MFTrainer: adam={adam!r}: expected 'lazy' or 'dense'")
        if objective == "bce":
            if group_size not in (None, 1):
                raise ValueError(f"MFTrainer: group_size={group_size!r}: the 'bce' objective has no groups")
            group_size = 1
        elif group_size is None or int(group_size) != group_size or not 2 <= group_size <= 64:
            raise ValueError(f"MFTrainer: group_size={group_size!r}: {objective!r} needs 1 + negatives, 2..64")
        if not (lr > 0 and np.isfinite(lr)) or not (reg >= 0 and np.isfinite(reg)):
            raise ValueError(f"MFTrainer: lr={lr!r} (> 0), reg={reg!r} (>= 0)")
        if len(betas) != 2 or not all(0 <= b < 1 for b in betas) or not eps > 0:
            raise ValueError(f"MFTrainer: betas={betas!r} (two values in [0, 1)), eps={eps!r} (> 0)")
        self.model, self.lr, self.reg, self.objective, self.G, self.adam = model, float(lr), float(reg), objective, int(group_size), adam
        self.b1, self.b2, self.eps, self.t = float(betas[0]), float(betas[1]), float(eps), 0
        dev, D = model.device, model.dim
        nu, ni = model.n_user * D, model.n_item * D
        self._m = torch.zeros(nu + ni, dtype=torch.float32, device=dev)
        self._v = torch.zeros(nu + ni, dtype=torch.float32, device=dev)
        self.m_user, self.m_item = self._m[:nu].view(-1, D), self._m[nu:].view(-1, D)
        self.v_user, self.v_item = self._v[:nu].view(-1, D), self._v[nu:].view(-1, D)
        self.status = torch.zeros(2, dtype=torch.int64, device=dev)       # lazy: (rows updated, entries dropped), accumulated
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)       # ranking: the pairwise-accuracy integers, accumulated
        self.last = None                                                  # (scores, dscore, du, di) of the last step
        if adam == "dense":
            self._g = torch.zeros(nu + ni, dtype=torch.float32, device=dev)
            table = np.zeros(2, dtype=[("x", "<u8"), ("off", "<i8"), ("n", "<i8"), ("l2", "<f4"), ("pad", "<i4")])   # mvin_param_seg
            table[0] = (model.user_emb_matrix.data_ptr(), 0, nu, 0.0, 0)
            table[1] = (model.entity_emb_matrix.data_ptr(), nu, ni, 0.0, 0)
            self._segs = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
            self._l2_sink = torch.zeros(1, dtype=torch.float32, device=dev)

    def lr_t(self, t):
        """The bias-corrected step size of step t (1-based): training.Trainer.lr_t's rule, as float32."""
        from .training import Trainer
        return float(np.float32(Trainer.lr_t(self, t)))

    def step(self, users, items, valid=None, labels=None):
        """One step.  "bce": ``users`` / ``items`` int64 [B], ``labels`` f32 [B], ``valid`` masks rows; the loss is the mean over
        the B rows.  Ranking: ``users`` int64 [n_groups], ``items`` int64 [n_groups, G] (or flat), ``valid`` f32 alike; the mean
        over the groups.  Returns (loss, reg_loss) as 0-d device tensors; enqueues only."""
        mdl, G = self.model, self.G
        U, V = mdl.user_emb_matrix, mdl.entity_emb_matrix
        if not torch.is_tensor(users) or not torch.is_tensor(items):
            raise ValueError("MFTrainer.step: users and items must be int64 device tensors")
        if self.objective == "bce" and labels is None:
            raise ValueError("MFTrainer.step: the 'bce' objective needs labels")
        if self.objective != "bce" and labels is not None:
            raise ValueError(f"MFTrainer.step: labels given with the {self.objective!r} objective")
        items = items.reshape(-1)
        valid = None if valid is None else valid.reshape(-1)
        n_groups = users.numel()
        if n_groups == 0:
            raise ValueError("MFTrainer.step: empty batch")
        acc = torch.zeros(2, dtype=torch.float32, device=mdl.device)
        self.last = ops.mf_head(U, V, users, items, self.objective, 1.0 / n_groups, self.reg, acc, group_size=G, valid=valid,
                                labels=labels, counts=None if self.objective == "bce" else self.counts)
        _, _, du, di = self.last
        self.t += 1
        lr_t = self.lr_t(self.t)
        ukeys = users if G == 1 else users.repeat_interleave(G)
        if self.adam == "lazy":
            if valid is not None and G > 1:                    # the head takes slot 0 whatever valid says: so does the optimiser
                valid = valid.view(-1, G).clone()
                valid[:, 0] = 1.0
                valid = valid.view(-1)
            ops.sparse_adam_rows(U, self.m_user, self.v_user, ukeys, du, lr_t, self.b1, self.b2, self.eps, self.status, valid=valid)
            ops.sparse_adam_rows(V, self.m_item, self.v_item, items, di, lr_t, self.b1, self.b2, self.eps, self.status, valid=valid)
        else:
            nu = U.numel()
            self._g.zero_()
            # a masked row's gradient is zero, so it adds nothing (ids are clamped as the head clamps them)
            ops.scatter_add_rows(self._g[:nu].view_as(U), ukeys.clamp(0, mdl.n_user - 1), du)
            ops.scatter_add_rows(self._g[nu:].view_as(V), items.clamp(0, mdl.n_item - 1), di)
            ops.l2_adam_multi(self._segs, 2, self._g.numel(), self._g, self._m, self._v, self._l2_sink, True, lr_t,
                              self.b1, self.b2, self.eps)
        return acc[0], acc[1]


class MFFeeder(DeviceFeeder):
    """A ``DeviceFeeder`` over an ``MFModel``: scores, logits, score_grid, recommend, rank_positives, recommend_lists,
    rank_lists, similar_items, diversify_lists (V as the feature table) and everything built on them (ctr_eval_split,
    compare_ctr, full_ranking_eval, compare_models, ...) work by inheritance through ``model.forward_users``.  ``retrieve``
    defaults its queries to the user rows: MF is its own tower."""

    def __init__(self, model):
        if not isinstance(model, MFModel):
            raise ValueError(f"MFFeeder: model must be an MFModel, got {type(model).__name__}")
        self.model, self.uts, self.P = model, None, 0

    def user_vectors(self, users):
        """U[users], f32 [n, D] on the device."""
        return self.model.user_emb_matrix[_dev_ids(users, self.model.device)]

    def retrieve(self, users, n_cand, candidates, queries=None, history=None, cosine=False, exclude=None, max_pairs=1 << 26):
        """``DeviceFeeder.retrieve`` with ``queries`` defaulting to ``user_vectors(users)`` when neither ``queries`` nor
        ``history`` is given: the inner product ranked is then the model's own score."""
        if queries is None and history is None:
            if isinstance(exclude, dict):
                if torch.is_tensor(users) and users.is_cuda:
                    raise ValueError("retrieve: an exclusion record needs host users (or pass feeder.exclusion_csr(users, record))")
                exclude = self.exclusion_csr(users, exclude)
            queries = self.user_vectors(users).contiguous()
        return DeviceFeeder.retrieve(self, users, n_cand, candidates, queries=queries, history=history, cosine=cosine,
                                     exclude=exclude, max_pairs=max_pairs)

    def _refuse(self, name, why):
        raise ValueError(f"MFFeeder.{name}: {why}")

    def memories(self, users_dev):
        self._refuse("memories", "a matrix-factorisation model has no ripple sets")

    def scores_user(self, user, items):
        self._refuse("scores_user", "the shared-user form reads ripple sets, which a matrix-factorisation model has not; use scores")

    def explain(self, *args, **kwargs):
        self._refuse("explain", "there are no knowledge-graph attention paths in a matrix-factorisation score")

    def explain_memories(self, *args, **kwargs):
        self._refuse("explain_memories", "there are no ripple-set memories in a matrix-factorisation score")


def train_mf(train_data, n_user, n_item, *, dim=64, lr, reg, epochs, batch_size, objective="bce", n_neg=1, neg_dist="uniform",
             adam="lazy", seed=1, eval_data=None, log=None, device="cuda"):
    """Train an ``MFModel`` on ``train_data`` (int rows (user, item, label)).  "bce" trains on the rows as they are, fixed
    negatives included, in the permutation ``np.random.default_rng([seed, epoch]).permutation(n)`` of each epoch; "bpr" /
    "softmax" on ``data_prep.rank_groups`` of a ``NegativeSampler(ratio=n_neg, dist=neg_dist, seed=seed)`` -- fresh negatives
    every epoch, the groups permuted the same way.  The tables start from ``xavier_tables(seed=seed)``.  One record per epoch:
    ``epoch``, ``loss`` and ``reg_loss`` (means over the epoch's steps), ``pairwise_acc`` (ranking objectives), ``eval`` =
    ``ctr_eval_split`` of ``eval_data`` when given; ``log(record)`` is called with each.  One copy back per epoch.  Returns
    ``(model, records)``; with ``adam="lazy"`` a pure function of its arguments."""
    from . import data_prep
    from .ctr_eval import ctr_eval_split
    if objective not in OBJECTIVES:
        raise ValueError(f"train_mf: objective={objective!r}: expected one of {OBJECTIVES}")
    epochs, batch_size, n_neg = int(epochs), int(batch_size), int(n_neg)
    if epochs < 0 or batch_size < 1:
        raise ValueError(f"train_mf: epochs={epochs} (>= 0), batch_size={batch_size} (>= 1)")
    if objective != "bce" and not 1 <= n_neg <= 63:
        raise ValueError(f"train_mf: n_neg={n_neg}: expected 1 .. 63")
    rows = np.asarray(train_data, dtype=np.int64).reshape(-1, 3)
    if rows.shape[0] == 0:
        raise ValueError("train_mf: empty train_data")
    model = MFModel(n_user, n_item, dim, seed=seed, device=device)
    dev = model.device
    tr = MFTrainer(model, lr, reg=reg, objective=objective, group_size=None if objective == "bce" else 1 + n_neg, adam=adam)
    feeder = MFFeeder(model)
    if objective == "bce":
        users = torch.from_numpy(np.ascontiguousarray(rows[:, 0])).to(dev)
        items = torch.from_numpy(np.ascontiguousarray(rows[:, 1])).to(dev)
        labels = torch.from_numpy(rows[:, 2].astype(np.float32)).to(dev)
        valid = None
    else:
        sampler = data_prep.NegativeSampler(rows, n_user, n_item, ratio=n_neg, seed=seed, device=dev, dist=neg_dist)
    records = []
    for epoch in range(epochs):
        if objective != "bce":
            users, items, valid = data_prep.rank_groups(sampler, epoch)
        n = users.shape[0]
        perm = torch.from_numpy(np.random.default_rng([int(seed), epoch]).permutation(n)).to(dev)
        sums = torch.zeros(2, dtype=torch.float32, device=dev)
        tr.counts.zero_()
        steps = 0
        for s0 in range(0, n, batch_size):
            idx = perm[s0:s0 + batch_size]
            if objective == "bce":
                loss, rl = tr.step(users[idx], items[idx], labels=labels[idx])
            else:
                loss, rl = tr.step(users[idx], items[idx].contiguous(), valid=valid[idx].contiguous())
            sums[0] += loss
            sums[1] += rl
            steps += 1
        host = torch.cat([sums.double(), tr.counts.double()]).cpu().numpy()
        rec = dict(epoch=epoch, loss=float(host[0] / steps), reg_loss=float(host[1] / steps))
        if objective != "bce":
            rec["pairwise_acc"] = float(host[2] / (2.0 * host[3])) if host[3] > 0 else float("nan")
        if eval_data is not None:
            rec["eval"] = ctr_eval_split(feeder, eval_data)
        records.append(rec)
        if log is not None:
            log(rec)
    return model, records
