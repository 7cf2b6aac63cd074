"""Harness counterpart: the callers of the scoring path in the reference
(src/model/MVIN/train.py:112-146, util.py:14-242), restated for the mvin_amd.MVIN model.

Scope row f-3 / f-4 of SURVEY.md section 8: feed assembly, CTR evaluation, top-K evaluation
and the attention case-study dump.  The epoch loop, early stopping and log book-keeping
(train.py:16-109, train_util.py) are not rebuilt.  Behaviours kept on purpose:

  * CTR eval walks FULL batches only and drops the ragged tail (util.py:49); metrics are
    means of per-batch AUC / ACC / F1 (util.py:56);
  * top-K eval scores every (user, item not in the user's train record) pair in batches of
    ``batch_size``, padding the last batch with its last item (util.py:166-177);
  * the NDCG hit list is built with the LAST k of ``k_list`` (the stale loop variable of
    util.py:187-199), i.e. over the top-100 items, then cut at each k inside ndcg_at_k.

``DeviceFeeder`` is the MI355X-first variant of the feed assembly: the ripple sets of all
users live on the GPU once ([n_user, P, 3, Nm] int32) and a batch's memories are gathered there,
so the per-step host work of train.py:117-120 (3*P python lists of B numpy rows) disappears.
"""
import numpy as np

from .ctr_eval import (CTR_ROW_METRICS, Calibration, OperatingPoint, compare_ctr, ctr_cluster_columns,  # noqa: F401
                       ctr_compare_pairs, ctr_compare_table, ctr_curves, ctr_eval_batched, ctr_eval_split, ctr_operating_points,
                       ctr_report, ctr_row_table, fit_calibration, pick_threshold, platt_fit)
from .ctr_eval import _check_criterion, _copy_back, ctr_report as _ctr_report    # train() takes an option named ctr_report


# --------------------------------------------------------------------------- feed assembly
def get_feed_dict(args, model, data, user_triplet_set, start, end):
    """train.py:112-122 / util.py:208-218."""
    feed = {model.user_indices: data[start:end, 0],
            model.item_indices: data[start:end, 1],
            model.labels: data[start:end, 2]}
    for i in range(max(1, args.p_hop)):
        feed[model.memories_h[i]] = [user_triplet_set[u][i][0] for u in data[start:end, 0]]
        feed[model.memories_r[i]] = [user_triplet_set[u][i][1] for u in data[start:end, 0]]
        feed[model.memories_t[i]] = [user_triplet_set[u][i][2] for u in data[start:end, 0]]
    return feed


def get_feed_dict_top_k(args, model, user_list, item, label, user_triplet_set):
    """train.py:124-134 / util.py:220-230."""
    feed = {model.user_indices: user_list, model.item_indices: item, model.labels: label}
    for i in range(max(1, args.p_hop)):
        feed[model.memories_h[i]] = [user_triplet_set[u][i][0] for u in user_list]
        feed[model.memories_r[i]] = [user_triplet_set[u][i][1] for u in user_list]
        feed[model.memories_t[i]] = [user_triplet_set[u][i][2] for u in user_list]
    return feed


def get_user_record(data, is_train=True):
    """train.py:136-146: user -> set of items with label 1."""
    rec = {}
    for u, i, lab in zip(data[:, 0], data[:, 1], data[:, 2]):
        if lab == 1:
            rec.setdefault(u, set()).add(i)
    return rec


class DeviceFeeder(object):
    """Ripple sets resident on the GPU; batches assembled by device-side row selection."""

    def __init__(self, model, user_triplet_set):
        import torch
        self.model = model
        if torch.is_tensor(user_triplet_set):   # already [n_user, P, 3, n_memory] (data_prep.get_user_triplet_set)
            self.uts = user_triplet_set.to(model.device).to(torch.int32).contiguous()
            self.P = self.uts.shape[1]
            return
        arr = np.asarray(user_triplet_set) if not isinstance(user_triplet_set, dict) else None
        if arr is None:  # dict user -> [P,3,Nm] (the reference's defaultdict)
            n_user = model.n_user
            some = next(iter(user_triplet_set.values()))
            arr = np.zeros((n_user,) + np.asarray(some).shape, dtype=np.int32)
            for u, v in user_triplet_set.items():
                arr[u] = v
        self.model = model
        self.uts = torch.from_numpy(np.ascontiguousarray(arr.astype(np.int32))).to(model.device)
        self.P = self.uts.shape[1]

    def memories(self, users_dev):
        sel = self.uts[users_dev.long()]
        return ([sel[:, i, 0].contiguous() for i in range(self.P)],
                [sel[:, i, 1].contiguous() for i in range(self.P)],
                [sel[:, i, 2].contiguous() for i in range(self.P)])

    def scores(self, users, items):
        """sigmoid scores of (users[i], items[i]) as a device tensor; inputs numpy or tensors."""
        import torch
        dev = self.model.device
        u = torch.as_tensor(np.asarray(users) if not torch.is_tensor(users) else users).to(dev).long()
        it = torch.as_tensor(np.asarray(items) if not torch.is_tensor(items) else items).to(dev).long()
        return self.model.forward_users(u, it, self.uts).scores_normalized     # feeds assembled inside the kernels

    def _forward_pairs(self, users, items):
        """The ``forward_users`` call ``scores`` makes, whole: its ``.scores`` are the logits, ``.scores_normalized`` their
        sigmoid."""
        import torch
        dev = self.model.device
        u = torch.as_tensor(np.asarray(users) if not torch.is_tensor(users) else users).to(dev).long()
        it = torch.as_tensor(np.asarray(items) if not torch.is_tensor(items) else items).to(dev).long()
        return self.model.forward_users(u, it, self.uts)

    def logits(self, users, items):
        """raw scores (the logits ``scores`` takes the sigmoid of) of (users[i], items[i]) as a device tensor: the ``.scores``
        of the same ``forward_users`` call."""
        return self._forward_pairs(users, items).scores

    def scores_user(self, user, items):
        """sigmoid scores of ONE user against ``items``: the shared-user form of the path (the
        user's ripple sets are read once per call, not once per pair)."""
        import torch
        dev = self.model.device
        it = torch.as_tensor(np.asarray(items) if not torch.is_tensor(items) else items).to(dev).long()
        sel = self.uts[int(user)]                                   # [P, 3, Nm]
        u = torch.full((1,), int(user), dtype=torch.int64, device=dev)
        return self.model.forward_device(u, it, [sel[i, 0].contiguous() for i in range(self.P)],
                                         [sel[i, 1].contiguous() for i in range(self.P)],
                                         [sel[i, 2].contiguous() for i in range(self.P)]).scores_normalized


    def score_grid(self, users, candidates, out=None):
        """sigmoid scores of every (users[i], candidates[j]) pair as a device tensor [U, N] (``out`` if given): the pair list is
        built on the device and scored by ONE ``forward_users`` call, in whatever form the model's automatic rules pick."""
        import torch
        dev = self.model.device
        u = _dev_ids(users, dev)
        it = _dev_ids(candidates, dev)
        U, N = u.shape[0], it.shape[0]
        if out is None:
            out = torch.empty((U, N), dtype=torch.float32, device=dev)
        if U == 0 or N == 0:
            return out
        sig = self.model.forward_users(u.repeat_interleave(N), it.repeat(U), self.uts, distinct_users=U).scores_normalized
        out.copy_(sig.view(U, N))
        return out

    def exclusion_csr(self, users, record):
        """Row i = the items of ``record[users[i]]`` (a get_user_record dict; a missing user has an empty row), ascending, as a
        device CSR pair (ptr int64 [U+1], ids int32) for ops.topk_rows / recommend.  Host plumbing, built once per call."""
        import torch
        ptr, ids = _exclusion_csr_host(users, record)
        dev = self.model.device
        return torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev)

    def recommend(self, users, k, candidates, exclude=None, max_pairs=524288):
        """The ``k`` best candidates of every user: (items int64 [U, k], scores f32 [U, k]) on the device, best first; equal scores
        keep the order of ``candidates`` (pass them ascending for the reference's tie order); rows with fewer than ``k`` eligible
        candidates end in item -1, score -inf.  ``exclude``: a get_user_record dict (``users`` then on the host) or an
        ``exclusion_csr`` pair.  Users are scored in chunks of at most ``max_pairs`` pairs (``score_grid``); a candidate list longer
        than ``max_pairs`` is also cut into column blocks whose running top-K is carried through ops.topk_rows.  Enqueues only:
        no synchronisation, no copy to the host."""
        import torch
        from . import ops
        dev = self.model.device
        k, max_pairs = int(k), int(max_pairs)
        if max_pairs < 1:
            raise ValueError(f"max_pairs={max_pairs}")
        if isinstance(exclude, dict):
            if torch.is_tensor(users) and users.is_cuda:
                raise ValueError("recommend: an exclusion record needs host users (or pass feeder.exclusion_csr(users, record))")
            exclude = self.exclusion_csr(users, exclude)
        u = _dev_ids(users, dev)
        U = u.shape[0]
        contiguous, base = False, 0
        if torch.is_tensor(candidates):
            cand = candidates.to(dev).long().reshape(-1)
            N = cand.shape[0]
        else:
            arr = np.asarray(candidates, dtype=np.int64).reshape(-1)
            N = arr.shape[0]
            # a contiguous id range (the full catalogue): the kernel derives each column's id from its position
            contiguous = bool(N and arr[0] >= 0 and arr[-1] < (1 << 31) - 1 and np.array_equal(arr, np.arange(arr[0], arr[0] + N)))
            base = int(arr[0]) if contiguous else 0
            cand = torch.from_numpy(arr).to(dev)
        cand_ids = None if contiguous else cand.to(torch.int32)
        out_ids = torch.empty((U, k), dtype=torch.int32, device=dev)
        out_vals = torch.empty((U, k), dtype=torch.float32, device=dev)
        if U == 0:
            return out_ids.long(), out_vals
        cols = max(1, min(N, max_pairs))
        per = max(1, max_pairs // cols)
        for u0 in range(0, U, per):
            u1 = min(U, u0 + per)
            out = (out_ids[u0:u1], out_vals[u0:u1])
            excl = None if exclude is None else (exclude[0][u0:u1 + 1], exclude[1])
            carry = None
            for c0 in range(0, N, cols) if N else [0]:
                c1 = min(N, c0 + cols)
                grid = self.score_grid(u[u0:u1], cand[c0:c1])
                ops.topk_rows(grid, k, cand_ids=None if cand_ids is None else cand_ids[c0:c1], col_offset=base + c0,
                              excl=excl, carry=carry, out=out)
                carry = out
        return out_ids.long(), out_vals

    def rank_positives(self, users, positives, candidates, exclude=None, max_pairs=524288):
        """Where every user's ``positives`` land in the user's ranking of ``candidates``, without ranking them: the device
        tensors ``(pos_ptr int64 [U+1], pos_ids int32 [T], counts int32 [T, 3], vals f32 [T], eligible int32 [U])`` of
        ops.rank_positives -- per positive (greater, equal_before, equal_after) among the user's eligible candidates and its
        score, (-1, -1, -1) / NaN when it is no candidate or excluded; equal scores rank in the order of ``candidates``, as in
        ``recommend``.  ``positives`` and ``exclude``: a get_user_record dict (``users`` then on the host) or an
        ``exclusion_csr`` pair.  Users are taken in chunks of max(1, max_pairs // N) rows; a chunk's scores fill one [rows, N]
        buffer through ``score_grid`` calls of at most ``max_pairs`` pairs each (column blocks when N > max_pairs), then ONE
        mvin_rank_positives call ranks the chunk.  Enqueues only: no synchronisation, no copy to the host."""
        import torch
        from . import ops
        dev = self.model.device
        max_pairs = int(max_pairs)
        if max_pairs < 1:
            raise ValueError(f"max_pairs={max_pairs}")
        for rec in (positives, exclude):
            if isinstance(rec, dict) and torch.is_tensor(users) and users.is_cuda:
                raise ValueError("rank_positives: a record needs host users (or pass feeder.exclusion_csr(users, record))")
        if isinstance(positives, dict):
            positives = self.exclusion_csr(users, positives)
        if isinstance(exclude, dict):
            exclude = self.exclusion_csr(users, exclude)
        pos_ptr, pos_ids = positives
        u = _dev_ids(users, dev)
        U = u.shape[0]
        cand, cand_ids, base = _candidate_ids(candidates, dev)
        N = cand.shape[0]
        T = pos_ids.numel()
        counts = torch.empty((T, 3), dtype=torch.int32, device=dev)
        vals = torch.empty((T,), dtype=torch.float32, device=dev)
        eligible = torch.empty((U,), dtype=torch.int32, device=dev)
        per = max(1, max_pairs // max(1, N))
        buf = torch.empty((min(per, U), N), dtype=torch.float32, device=dev)
        for u0 in range(0, U, per):
            u1 = min(U, u0 + per)
            grid = buf[:u1 - u0]
            cols = max(1, max_pairs // (u1 - u0))
            if cols >= N:
                self.score_grid(u[u0:u1], cand, out=grid)
            else:
                for c0 in range(0, N, cols):
                    c1 = min(N, c0 + cols)
                    self.score_grid(u[u0:u1], cand[c0:c1], out=grid[:, c0:c1])
            ops.rank_positives(grid, (pos_ptr[u0:u1 + 1], pos_ids), cand_ids=cand_ids, col_offset=base,
                               excl=None if exclude is None else (exclude[0][u0:u1 + 1], exclude[1]),
                               out=(counts, vals, eligible[u0:u1]))
        return pos_ptr, pos_ids, counts, vals, eligible

    def _score_lists(self, u, ptr, items, max_pairs):
        """sigmoid scores of the expanded pair list (user i repeated over its list) as one flat device tensor [T]:
        ``forward_users`` calls of at most ``max_pairs`` pairs each, ``distinct_users`` = the lists a piece touches."""
        import torch
        dev = self.model.device
        T = int(ptr[-1])
        flat = torch.empty((T,), dtype=torch.float32, device=dev)
        if T == 0:
            return flat
        lens = torch.from_numpy(np.diff(ptr)).to(dev)
        u_exp = u.repeat_interleave(lens, output_size=T)
        for a in range(0, T, max_pairs):
            b = min(T, a + max_pairs)
            touched = int(np.searchsorted(ptr, b, side="left") - np.searchsorted(ptr, a, side="right") + 1)
            flat[a:b] = self.model.forward_users(u_exp[a:b], items[a:b], self.uts, distinct_users=touched).scores_normalized
        return flat

    def recommend_lists(self, users, lists, k, exclude=None, max_pairs=524288):
        """The ``k`` best items of every user's OWN candidate list -- the reranking stage of a two-stage recommender:
        ``(items int64 [U, k], scores f32 [U, k], positions int32 [U, k])`` on the device, best first, ``positions`` the places
        inside the user's list; equal scores keep the list's order; a list with fewer than ``k`` eligible items ends in item -1,
        score -inf, position -1.  ``lists``: a CSR pair (a tuple ``(ptr [U+1], items [T])``, host or device) or a Python list of
        per-user arrays; a negative item id is padding.  ``exclude`` as in ``recommend``.  The expanded pair list is scored into
        one flat buffer in pieces of at most ``max_pairs`` pairs (a piece may cut a list), then ops.topk_segments runs once per
        chunk of whole lists holding at most ``max_pairs`` pairs (one list when it is longer), with the chunk's own longest list
        as the bound -- a chunk of short lists takes the wave form whatever another chunk holds.  Device pointers are copied to
        the host once to cut the chunks; beyond that the call only enqueues: no copy back of any result."""
        import torch
        from . import ops
        dev = self.model.device
        k, max_pairs = int(k), int(max_pairs)
        if max_pairs < 1:
            raise ValueError(f"max_pairs={max_pairs}")
        if isinstance(exclude, dict):
            if torch.is_tensor(users) and users.is_cuda:
                raise ValueError("recommend_lists: an exclusion record needs host users (or pass feeder.exclusion_csr(users, record))")
            exclude = self.exclusion_csr(users, exclude)
        u = _dev_ids(users, dev)
        U = u.shape[0]
        ptr, items = _lists_csr(lists, U, dev)
        flat = self._score_lists(u, ptr, items.clamp(min=0), max_pairs)      # padding is scored as item 0 and never eligible
        ids = items.to(torch.int32)
        seg_ptr = torch.from_numpy(ptr).to(dev)
        out = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev),
               torch.empty((U, k), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
        for s0, s1, longest in _segment_chunks(ptr, max_pairs):
            ops.topk_segments(flat, seg_ptr[s0:s1 + 1], k, ids=ids,
                              excl=None if exclude is None else (exclude[0][s0:s1 + 1], exclude[1]), max_len=longest,
                              out=(out[0][s0:s1], out[1][s0:s1], out[2][s0:s1], out[3]))
        return out[2].long(), out[1], out[0]

    def diversify_lists(self, users, lists, k, lam=0.5, features=None, cosine=True, exclude=None, max_pairs=524288):
        """``recommend_lists`` with a trade-off between relevance and redundancy inside the returned list: greedy maximal marginal
        relevance (ops.mmr_segments).  Slot t of a user's list is the eligible item not taken yet with the largest
        ``lam * score - (1 - lam) * (largest similarity to an item already taken)``; ``lam=1.0`` is ``recommend_lists`` bit for
        bit, ``lam=0.0`` ignores the scores after the first pick.  Similarity is the dot product of two rows of ``features`` (an
        f32 [n_rows, D] device table indexed by item id, D a multiple of 4 in 4..256; None = ``model.entity_emb_matrix``, where
        the items are the low entity ids; a bf16 table raises ValueError), a cosine with ``cosine=True`` (the inverse row norms
        are computed once per call on the device, ops.row_inv_norms).  ``lists``, ``exclude`` and ``max_pairs`` as in
        ``recommend_lists``, scored and chunked the same way; an item id beyond the table is never eligible; a list longer than
        ops.mmr_max_len() raises ValueError.  Returns ``(items int64 [U, k], scores f32 [U, k], positions int32 [U, k], penalties
        f32 [U, k], simsums f32 [U, k])`` on the device: per slot the item, its score, its place in the user's list, the
        similarity penalty it was taken at (0 in slot 0) and the sum of its similarities to the slots before it -- a list's
        mean pairwise similarity is ``simsums.sum() / (m (m - 1) / 2)`` over its m picks.  A list with fewer than ``k`` eligible
        items ends in item -1, score -inf, position -1 and zeros.  Nothing is copied back."""
        import torch
        from . import ops
        dev = self.model.device
        k, max_pairs = int(k), int(max_pairs)
        if max_pairs < 1:
            raise ValueError(f"max_pairs={max_pairs}")
        feat = self.model.entity_emb_matrix if features is None else features
        if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 2:
            raise ValueError(f"diversify_lists: features must be an f32 [n_rows, D] table, got "
                             f"{feat.dtype if torch.is_tensor(feat) else type(feat).__name__} (a bf16 table is not taken)")
        if isinstance(exclude, dict):
            if torch.is_tensor(users) and users.is_cuda:
                raise ValueError("diversify_lists: an exclusion record needs host users (or pass feeder.exclusion_csr(users, record))")
            exclude = self.exclusion_csr(users, exclude)
        u = _dev_ids(users, dev)
        U = u.shape[0]
        ptr, items = _lists_csr(lists, U, dev)
        lens = np.diff(ptr)
        if lens.size and int(lens.max()) > ops.mmr_max_len():
            i = int(np.argmax(lens > ops.mmr_max_len()))
            raise ValueError(f"diversify_lists: the list of user {int(u[i])} (row {i}) has {int(lens[i])} entries, "
                             f"more than ops.mmr_max_len() = {ops.mmr_max_len()}")
        feat = feat.to(dev)
        row_scale = ops.row_inv_norms(feat) if cosine else None
        flat = self._score_lists(u, ptr, items.clamp(min=0), max_pairs)      # padding is scored as item 0 and never eligible
        ids = items.clamp(min=-1, max=(1 << 31) - 1).to(torch.int32)         # an id int32 cannot hold is beyond every table
        seg_ptr = torch.from_numpy(ptr).to(dev)
        pos, vals, oid, pen, simsum = (torch.empty((U, k), dtype=dt, device=dev)
                                       for dt in (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32))
        status = torch.zeros(2, dtype=torch.int64, device=dev)
        for s0, s1, longest in _segment_chunks(ptr, max_pairs):
            ops.mmr_segments(flat, seg_ptr[s0:s1 + 1], ids, feat, k, lam, row_scale=row_scale,
                             excl=None if exclude is None else (exclude[0][s0:s1 + 1], exclude[1]), max_len=longest,
                             out=(pos[s0:s1], vals[s0:s1], oid[s0:s1], None, pen[s0:s1], simsum[s0:s1], status))
        return oid.long(), vals, pos, pen, simsum

    def _retrieval_table(self, name):
        """The item rows retrieval scores against: ``model.entity_emb_matrix`` (the items are the low entity ids), f32 only."""
        import torch
        feat = self.model.entity_emb_matrix
        if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 2:
            raise ValueError(f"{name}: the entity table must be an f32 [n_rows, D] tensor, got "
                             f"{feat.dtype if torch.is_tensor(feat) else type(feat).__name__} (a bf16 table is not taken)")
        return feat.detach()

    def user_queries(self, users, history):
        """The default retrieval query of every user, f32 [U, D] on the device: the mean entity embedding of the user's
        positive train items (ops.mean_rows_segments: summed in f64 in interaction order, rounded once, bit-reproducible).
        ``history`` is a ``data_prep.history_csr`` pair (ptr int64 [n_user + 1], items int32) on the device; the means of all
        its users are built and the rows of ``users`` taken.  A user without history gets a ZERO row: every item then scores
        0 and ``retrieve`` returns the first eligible candidates in candidate order.  This query is a PROXY: MVIN's own user
        vector depends on the item it is scored against, so nothing guarantees that the proxy keeps MVIN's top-k
        (``retrieval_eval`` measures how much it keeps).  Enqueues only."""
        from . import ops
        if not isinstance(history, tuple) or len(history) != 2:
            raise ValueError("user_queries: history must be a data_prep.history_csr pair (ptr, items)")
        feat = self._retrieval_table("user_queries")
        u = _dev_ids(users, self.model.device)
        return ops.mean_rows_segments(feat, history[0], history[1])[u]

    def retrieve(self, users, n_cand, candidates, queries=None, history=None, cosine=False, exclude=None, max_pairs=1 << 26):
        """First-stage retrieval: every user's ``n_cand`` best candidates by inner product between a query vector and the items'
        entity embeddings, ``(items int64 [U, n_cand], sims f32 [U, n_cand])`` on the device, best first, equal similarities in
        the order of ``candidates``, rows short of ``n_cand`` eligible items ending in item -1, similarity -inf
        (ops.mips_topk: the fused kernel for n_cand <= ops.mips_topk_max_k(), the composed form up to 1024).  ``queries``:
        an f32 [U, D] device tensor of the caller's own tower; otherwise ``history`` (``user_queries``) is required.
        ``cosine=True`` divides by both norms (ops.row_inv_norms).  ``candidates`` and ``exclude`` mean what they mean in
        ``recommend``: a host list that is a contiguous id range takes the implicit-id path, ``exclude`` is a get_user_record
        dict (``users`` then on the host) or an ``exclusion_csr`` pair.  A candidate id outside the entity table is never
        returned.  ``max_pairs`` bounds the score buffer of the composed form.  Enqueues only."""
        import torch
        from . import ops
        dev = self.model.device
        n_cand = int(n_cand)
        if not 1 <= n_cand <= 1024:
            raise ValueError(f"retrieve: n_cand={n_cand}: expected 1 .. 1024")
        if int(max_pairs) < 1:
            raise ValueError(f"max_pairs={max_pairs}")
        if queries is None and history is None:
            raise ValueError("retrieve: pass queries ([U, D] f32) or history (a data_prep.history_csr pair)")
        if isinstance(exclude, dict):
            if torch.is_tensor(users) and users.is_cuda:
                raise ValueError("retrieve: an exclusion record needs host users (or pass feeder.exclusion_csr(users, record))")
            exclude = self.exclusion_csr(users, exclude)
        feat = self._retrieval_table("retrieve")
        u = _dev_ids(users, dev)
        U = u.shape[0]
        if queries is None:
            q = self.user_queries(u, history)
        else:
            if not torch.is_tensor(queries) or queries.dtype != torch.float32 or tuple(queries.shape) != (U, feat.shape[1]):
                raise ValueError(f"retrieve: queries must be an f32 [{U}, {feat.shape[1]}] tensor")
            q = queries.to(dev).contiguous()
        cand_ids, base, N = _candidate_columns(candidates, dev)
        q_scale = row_scale = None
        if cosine:
            row_scale = ops.row_inv_norms(feat)
            q_scale = ops.row_inv_norms(q) if U else None
        ids, sims = ops.mips_topk(q, feat, n_cand, cand_ids=cand_ids, col_offset=base, n=None if cand_ids is not None else N,
                                  q_scale=q_scale, row_scale=row_scale, excl=exclude, max_scores=int(max_pairs))
        return ids.long(), sims

    def recommend_two_stage(self, users, k, n_cand, candidates, queries=None, history=None, cosine=False, exclude=None,
                            max_pairs=524288, retriever=None):
        """``retrieve`` followed by ``recommend_lists`` on the retrieved lists: the model scores ``n_cand`` items per user, not
        the catalogue.  Arguments as in ``retrieve`` (``max_pairs`` is ``recommend_lists``'); the -1 padding of a short
        retrieved list is ``recommend_lists``' padding.  Returns what ``recommend_lists`` returns, ``positions`` being places
        in the user's retrieved list.  With ``n_cand`` at least the user's eligible candidates the item set is ``recommend``'s.
        Nothing is copied back.  ``retriever`` (None: this feeder's own ``retrieve``, as above): any object with a
        ``retrieve(users, n_cand, candidates, exclude=...)`` method returning ``(items int64 [U, n_cand], sims)`` -- a learned
        tower such as ``mf.MFFeeder`` -- runs the first stage instead; ``queries`` / ``history`` / ``cosine`` are then not used."""
        k, n_cand = int(k), int(n_cand)
        if retriever is not None:
            items, _ = retriever.retrieve(users, n_cand, candidates, exclude=exclude)
        else:
            items, _ = self.retrieve(users, n_cand, candidates, queries=queries, history=history, cosine=cosine, exclude=exclude)
        U = items.shape[0]
        ptr = np.arange(U + 1, dtype=np.int64) * n_cand
        return self.recommend_lists(users, (ptr, items.reshape(-1)), k, max_pairs=max_pairs)

    def similar_items(self, items, k, candidates, cosine=True):
        """Item-to-item neighbours: for every item of ``items`` (rows of the entity table) the ``k`` candidates whose entity
        embedding has the largest cosine (``cosine=False``: inner product) with the item's own, the item itself excluded
        through a one-id exclusion row: ``(neighbours int64 [n, k], sims f32 [n, k])`` on the device.  ``candidates`` as in
        ``recommend``.  Enqueues only."""
        import torch
        from . import ops
        dev = self.model.device
        k = int(k)
        if not 1 <= k <= 1024:
            raise ValueError(f"similar_items: k={k}: expected 1 .. 1024")
        feat = self._retrieval_table("similar_items")
        if not torch.is_tensor(items):
            arr = np.asarray(items, dtype=np.int64).reshape(-1)
            if arr.size and (arr.min() < 0 or arr.max() >= feat.shape[0]):
                raise ValueError(f"similar_items: item ids must be rows of the entity table (0 .. {feat.shape[0] - 1})")
        it = _dev_ids(items, dev)
        n = it.shape[0]
        q = feat[it.clamp(0, max(feat.shape[0] - 1, 0))].contiguous()
        excl = (torch.arange(n + 1, dtype=torch.int64, device=dev), it.to(torch.int32))
        cand_ids, base, N = _candidate_columns(candidates, dev)
        q_scale = row_scale = None
        if cosine:
            row_scale = ops.row_inv_norms(feat)
            q_scale = row_scale[it.clamp(0, max(feat.shape[0] - 1, 0))].contiguous()
        ids, sims = ops.mips_topk(q, feat, k, cand_ids=cand_ids, col_offset=base, n=None if cand_ids is not None else N,
                                  q_scale=q_scale, row_scale=row_scale, excl=excl)
        return ids.long(), sims

    def rank_lists(self, users, lists, queries, exclude=None, max_pairs=524288):
        """Where named entries of every user's OWN candidate list land in the user's ranking of that list: the device tensors
        ``(q_ptr int64 [U+1], q_pos int32 [Q], counts int32 [Q, 3], vals f32 [Q], eligible int32 [U])`` of ``rank_positives``,
        through ops.rank_segments.  ``lists`` and ``exclude`` as in ``recommend_lists``; ``queries`` names POSITIONS inside the
        lists: a CSR pair (a tuple ``(q_ptr [U+1], q_pos [Q])``) or a Python list of per-user arrays, each ascending and
        distinct.  A position beyond its list, or at a padded or excluded item, gets (-1, -1, -1) and NaN.  Scored and chunked
        as ``recommend_lists`` does it; nothing is copied back."""
        import torch
        from . import ops
        dev = self.model.device
        max_pairs = int(max_pairs)
        if max_pairs < 1:
            raise ValueError(f"max_pairs={max_pairs}")
        if isinstance(exclude, dict):
            if torch.is_tensor(users) and users.is_cuda:
                raise ValueError("rank_lists: an exclusion record needs host users (or pass feeder.exclusion_csr(users, record))")
            exclude = self.exclusion_csr(users, exclude)
        u = _dev_ids(users, dev)
        U = u.shape[0]
        ptr, items = _lists_csr(lists, U, dev)
        q_ptr_h, q_pos = _lists_csr(queries, U, dev)
        q_ptr, q_pos = torch.from_numpy(q_ptr_h).to(dev), q_pos.to(torch.int32)
        flat = self._score_lists(u, ptr, items.clamp(min=0), max_pairs)
        ids = items.to(torch.int32)
        seg_ptr = torch.from_numpy(ptr).to(dev)
        Q = q_pos.numel()
        out = (torch.empty((Q, 3), dtype=torch.int32, device=dev), torch.empty((Q,), dtype=torch.float32, device=dev),
               torch.empty((U,), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
        for s0, s1, longest in _segment_chunks(ptr, max_pairs):
            ops.rank_segments(flat, seg_ptr[s0:s1 + 1], (q_ptr[s0:s1 + 1], q_pos), ids=ids,
                              excl=None if exclude is None else (exclude[0][s0:s1 + 1], exclude[1]), max_len=longest,
                              out=(out[0], out[1], out[2][s0:s1], out[3]))
        return q_ptr, q_pos, out[0], out[1], out[2]

    def explain(self, users, items, top=10, profile=False, return_attention=False, max_pairs=65536):
        """Which knowledge-graph paths carried the score of every pair (users[i], items[i]), and how much of it: the attention
        outputs of the i = 0 pass merged and ranked on the device by ops.explain_paths (include/mvin_hip.h states the rule).  The
        sampler repeats slots whenever an entity has fewer than K edges, so a path item -rel0-> ent1 -rel1-> ent2 is spread over
        many of the K + K^2 slots the case study dumps; here slots with the same ids are ONE path with the integer sum of their
        masses floor(w0 * w1 * 2^40), listed mass descending, then lowest slot ascending -- an exact, reproducible order although
        ties are everywhere (the attention logit is one number per relation).  Returns a dict of device tensors:
          scores [B] f32 (sigmoid; the ``want_probs`` pass takes another kernel form than ``scores``, so they agree to rounding),
          paths [B, top, 4] int32 = (rel0, ent1, rel1, ent2), mass [B, top] int64, weight [B, top] f64 = mass / 2^40,
          slot [B, top] int32, distinct [B] int32, total [B] int64 (rows past ``distinct``: ids -1, mass 0, slot -1);
          ``profile=True``: rel_mass [2, n_relation] int64, the attention mass per relation at both levels, summed over the
          chunks in int64 (a pair adds at most 2^40 per level: exact below 2^23 pairs);
          ``return_attention=True``: imp0 [B, 1, K] and imp1 [B, K, K] (None at depth 1), the tensors the paths were cut from.
        A model of depth 1 (h_hop = 1) takes one-hop mode: the entries are the K level-1 slots, the last two path columns -1.
        With more than two levels the paths are those of the FIRST TWO, exactly what ``eval_case_study`` exposes.  The user side
        (key addressing) is explained by ``explain_memories``.  One ``forward_users(..., want_probs=True)`` and one
        ``get_neighbors`` per chunk of at most ``max_pairs`` pairs (fewer where the kernel's bounds ask for it: B * K^2 <= 2^22
        with ``profile``).  Enqueues only: nothing is copied back."""
        import torch
        from . import ops
        m = self.model
        dev = m.device
        u, it = _dev_ids(users, dev), _dev_ids(items, dev)
        if u.shape[0] != it.shape[0]:
            raise ValueError(f"explain: {u.shape[0]} users for {it.shape[0]} items")
        B, K, nR = u.shape[0], m.n_neighbor, m.n_relation
        two = m.n_mix_hop * m.h_hop >= 2
        N = K * K if two else K
        top, max_pairs = int(top), int(max_pairs)
        if max_pairs < 1 or not 1 <= top <= N:
            raise ValueError(f"explain: max_pairs={max_pairs}, top={top} (1 <= top <= {N} entries per pair)")
        if K > ops.explain_paths_max_k():
            raise ValueError(f"explain: fan-out K={K} is beyond mvin_explain_paths' {ops.explain_paths_max_k()}")
        chunk = max(1, min(max_pairs, (ops.EXPLAIN_PROFILE_SLOTS if profile else (1 << 31) - 1) // (K * K)))
        res = dict(scores=torch.empty((B,), dtype=torch.float32, device=dev),
                   paths=torch.empty((B, top, 4), dtype=torch.int32, device=dev),
                   mass=torch.empty((B, top), dtype=torch.int64, device=dev),
                   slot=torch.empty((B, top), dtype=torch.int32, device=dev),
                   distinct=torch.empty((B,), dtype=torch.int32, device=dev),
                   total=torch.empty((B,), dtype=torch.int64, device=dev))
        if profile:
            res["rel_mass"] = torch.zeros((2, nR), dtype=torch.int64, device=dev)
        att0, att1 = [], []
        for a in range(0, B, chunk):
            b = min(B, a + chunk)
            out = m.forward_users(u[a:b], it[a:b], self.uts, want_probs=True)
            imp = out.importance_list
            if not imp or imp[0] is None or (two and (len(imp) < 2 or imp[1] is None)):
                raise ValueError("explain: this model's aggregator gives no attention outputs (importance_list is empty: "
                                 "User_orient_rela off, or a pass without the i = 0 probabilities); there is nothing to explain")
            imp0, imp1 = imp[0], imp[1] if two else None
            ents, rels = m.get_neighbors(it[a:b], levels=2 if two else 1)
            part = torch.zeros((2, nR), dtype=torch.int64, device=dev) if profile else None
            ops.explain_paths(imp0, imp1, rels, ents, top, nR, rel_mass=part,
                              out=(res["paths"][a:b], res["mass"][a:b], res["slot"][a:b], res["distinct"][a:b], res["total"][a:b]))
            res["scores"][a:b] = out.scores_normalized
            if profile:
                res["rel_mass"] += part
            if return_attention:
                att0.append(imp0.reshape(b - a, 1, K))
                att1.append(imp1.reshape(b - a, K, K) if two else None)
        res["weight"] = res["mass"].to(torch.float64) / ops.EXPLAIN_SCALE
        if return_attention:
            res["imp0"] = torch.cat(att0) if att0 else torch.empty((0, 1, K), dtype=torch.float32, device=dev)
            res["imp1"] = (torch.cat(att1) if att1 else torch.empty((0, K, K), dtype=torch.float32, device=dev)) if two else None
        return res

    def explain_memories(self, users, items, top=10, profile=False, return_attention=False, max_pairs=4096):
        """Which of the user's ripple-set memories (h, r, t) the score of every pair (users[i], items[i]) was read from, and how
        much each gave: the user side of ``explain``.  The logit is additive over the memories -- with v' the pair's final item
        embedding and g = user_mlp_matrix . v', score = user_mlp_bias . v' + sum over blocks c and memories m of
        p[c,m] * (x[c,m] . g_c) -- so every memory has an attention mass AND a signed contribution to the logit, and the
        contributions plus the bias term are the score.  ops.explain_memories recomputes the attention of these pairs
        (include/mvin_hip.h states the rule): the sampler draws ripple sets with replacement, so slots with the same key (h in
        the h-set block, (h, r, t) in a hop block) are ONE memory with the integer sum of their masses floor(p * 2^40), listed
        per block mass descending, then lowest slot ascending.  Blocks are [h-set (with PS_O_ft) | hop 0 | .. | hop P-1], n_o of
        them.  Returns a dict of device tensors:
          scores [B] f32 (the raw logit of the forward pass) and scores_normalized [B] f32 (its sigmoid),
          score_parts [B, n_o + 1] f32 = [block .. | bias]: each block's share of the logit and the bias term; their sum is the
          logit evaluated another way, equal to ``scores`` up to float32 rounding,
          mem [B, n_o, top, 3] int32 = (h, r, t), (h, -1, -1) in the h-set block, mass [B, n_o, top] int64, weight f64 = mass / 2^40,
          contrib [B, n_o, top] f32, slot [B, n_o, top] int32, distinct [B, n_o] int32, total [B, n_o] int64, block [B, n_o] f32,
          bias [B] f32 (rows past ``distinct``: ids -1, mass 0, contribution 0, slot -1);
          ``profile=True``: rel_mass [P, n_relation] int64, the attention mass per relation and hop, summed over the chunks;
          ``return_attention=True``: probs and slot_contrib [B, n_o, Nm] f32, per slot.
        Masses are per-block softmaxes and rank inside a block only; contributions are comparable across blocks.  Refuses
        ``HO_only`` models (their user vector is the plain user embedding: no memory enters the score), ripple sets of more
        than ops.explain_memories_max_nm() memories and bf16 entity tables.  One ``forward_users`` call, the V and G projections
        and one kernel launch per chunk of at most ``max_pairs`` pairs.  Enqueues only: nothing is copied back."""
        import torch
        from . import ops
        m = self.model
        a = m.args
        if a.HO_only:
            raise ValueError("explain_memories: an HO_only model's user vector is the plain user embedding; no ripple-set memory "
                             "enters its score, so there is nothing to explain")
        if m.table_dtype == "bf16":
            raise ValueError("explain_memories: table_dtype='bf16' is not supported (mvin_explain_memories takes fp32 tables only)")
        P, Nm, D, nR = m.p_hop, m.n_memory, m.dim, m.n_relation
        has_set = bool(a.PS_O_ft)
        n_o = P + (1 if has_set else 0)
        top, max_pairs = int(top), int(max_pairs)
        if Nm > ops.explain_memories_max_nm():
            raise ValueError(f"explain_memories: n_memory={Nm} is beyond mvin_explain_memories' {ops.explain_memories_max_nm()}")
        if n_o < 1:
            raise ValueError("explain_memories: the model reads no ripple set (p_hop = 0 without PS_O_ft)")
        if max_pairs < 1 or not 1 <= top <= Nm:
            raise ValueError(f"explain_memories: max_pairs={max_pairs}, top={top} (1 <= top <= {Nm} memories per block)")
        dev = m.device
        u, it = _dev_ids(users, dev), _dev_ids(items, dev)
        if u.shape[0] != it.shape[0]:
            raise ValueError(f"explain_memories: {u.shape[0]} users for {it.shape[0]} items")
        B = u.shape[0]
        chunk = max(1, min(max_pairs, (ops.EXPLAIN_MEM_PROFILE_SLOTS if profile else (1 << 31) - 1) // (Nm * n_o)))
        f32, i32, i64 = torch.float32, torch.int32, torch.int64
        res = dict(scores=torch.empty((B,), dtype=f32, device=dev), scores_normalized=torch.empty((B,), dtype=f32, device=dev),
                   score_parts=torch.empty((B, n_o + 1), dtype=f32, device=dev),
                   mem=torch.empty((B, n_o, top, 3), dtype=i32, device=dev), mass=torch.empty((B, n_o, top), dtype=i64, device=dev),
                   contrib=torch.empty((B, n_o, top), dtype=f32, device=dev), slot=torch.empty((B, n_o, top), dtype=i32, device=dev),
                   distinct=torch.empty((B, n_o), dtype=i32, device=dev), total=torch.empty((B, n_o), dtype=i64, device=dev),
                   block=torch.empty((B, n_o), dtype=f32, device=dev), bias=torch.empty((B,), dtype=f32, device=dev))
        if return_attention:
            res["probs"] = torch.empty((B, n_o, Nm), dtype=f32, device=dev)
            res["slot_contrib"] = torch.empty((B, n_o, Nm), dtype=f32, device=dev)
        if profile:
            res["rel_mass"] = torch.zeros((P, nR), dtype=i64, device=dev)
        kernel_out = ops.EXPLAIN_MEM_OUT + (("probs", "slot_contrib") if return_attention else ())
        w_h = m.h_emb_item_mlp_matrix.view(-1) if has_set else None
        Wt = m.user_mlp_matrix.t().contiguous()                  # [D, n_o * D]: G = v' . W^T (the transpose is plumbing)
        E = m.entity_emb_matrix
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            out = m.forward_users(u[lo:hi], it[lo:hi], self.uts)
            v = out.item_embeddings.contiguous()
            V = None
            if P > 0:                                            # exactly as MVIN._key_addressing builds it
                V = torch.empty((hi - lo, nR, D), dtype=f32, device=dev)
                ops.linear([E], m.relation_emb_KGE_matrix, D, ids=[it[lo:hi]], rows=hi - lo, out=V, ldo=nR * D, nz=nR,
                           w_zstride=D * D, out_zstride=D)
            G = ops.linear([v], Wt, n_o * D)
            part = torch.zeros((P, nR), dtype=i64, device=dev) if profile else None
            ops.explain_memories(E, V, w_h, self.uts, u[lo:hi], G, m.user_mlp_bias, v, P, top, rel_mass=part,
                                 want_slots=return_attention, out={k: res[k][lo:hi] for k in kernel_out})
            res["scores"][lo:hi] = out.scores
            res["scores_normalized"][lo:hi] = out.scores_normalized
            if profile:
                res["rel_mass"] += part
        res["score_parts"][:, :n_o] = res["block"]
        res["score_parts"][:, n_o] = res["bias"]
        res["weight"] = res["mass"].to(torch.float64) / ops.EXPLAIN_SCALE
        return res


def _lists_csr(lists, U, dev):
    """(ptr int64 [U+1] on the HOST, entries int64 [T] on the device) of per-user lists given as a CSR pair (a tuple of ptr and
    entries, host or device: a device ptr is copied back once) or as a Python list of per-user arrays."""
    import torch
    if isinstance(lists, tuple):
        if len(lists) != 2:
            raise ValueError("lists: a CSR pair is a tuple (ptr, entries)")
        ptr, entries = lists
        ptr = np.ascontiguousarray(ptr.cpu().numpy() if torch.is_tensor(ptr) else np.asarray(ptr), dtype=np.int64).reshape(-1)
        entries = _dev_ids(entries, dev)
    else:
        rows = [np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64).reshape(-1) for r in lists]
        ptr = np.zeros(len(rows) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([r.size for r in rows])
        entries = torch.from_numpy(np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)).to(dev)
    if ptr.size != U + 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != entries.shape[0]:
        raise ValueError(f"lists: expected {U} lists whose pointers run from 0 to the {entries.shape[0]} entries")
    return ptr, entries


def _segment_chunks(ptr, max_pairs):
    """Cut segments 0 .. len(ptr) - 2 into runs of whole segments of at most ``max_pairs`` entries each (a longer segment is a
    run of its own): yields (first, one past the last, the run's longest segment)."""
    n, lens, s0 = ptr.size - 1, np.diff(ptr), 0
    while s0 < n:
        s1 = max(s0 + 1, int(np.searchsorted(ptr, ptr[s0] + max_pairs, side="right")) - 1)
        yield s0, s1, int(lens[s0:s1].max())
        s0 = s1


def _candidate_ids(candidates, dev):
    """(ids int64 [N] on the device, int32 ids per column or None, first id): a host list that is a contiguous id range (the full
    catalogue) needs no id per column, the kernels derive it from the position."""
    import torch
    if torch.is_tensor(candidates):
        cand = candidates.to(dev).long().reshape(-1)
        return cand, cand.to(torch.int32), 0
    arr = np.asarray(candidates, dtype=np.int64).reshape(-1)
    N = arr.shape[0]
    contiguous = bool(N and arr[0] >= 0 and arr[-1] < (1 << 31) - 1 and np.array_equal(arr, np.arange(arr[0], arr[0] + N)))
    cand = torch.from_numpy(arr).to(dev)
    return cand, None if contiguous else cand.to(torch.int32), int(arr[0]) if contiguous else 0


def _candidate_columns(candidates, dev):
    """(int32 ids per column on the device or None, first id, N) for the retrieval calls: ``_candidate_ids`` without the int64
    copy of the list on the device, which retrieval never reads; a ``range`` of step 1 is not even expanded on the host."""
    import torch
    if isinstance(candidates, range) and candidates.step == 1 and (len(candidates) == 0 or
                                                                   (candidates.start >= 0 and candidates.stop < (1 << 31))):
        return None, candidates.start if len(candidates) else 0, len(candidates)
    if torch.is_tensor(candidates):
        cand = candidates.to(dev).reshape(-1)
        return cand.clamp(-1, (1 << 31) - 1).to(torch.int32), 0, cand.shape[0]      # an id int32 cannot hold is beyond every table
    arr = np.asarray(candidates, dtype=np.int64).reshape(-1)
    N = arr.shape[0]
    if N and arr[0] >= 0 and arr[-1] < (1 << 31) - 1 and arr[-1] - arr[0] == N - 1 and np.array_equal(arr, np.arange(arr[0], arr[0] + N)):
        return None, int(arr[0]), N
    return torch.from_numpy(np.clip(arr, -1, (1 << 31) - 1).astype(np.int32)).to(dev), 0, N


def _dev_ids(x, dev):
    import torch
    if torch.is_tensor(x):
        return x.to(dev).long().reshape(-1)
    return torch.from_numpy(np.asarray(x, dtype=np.int64).reshape(-1)).to(dev)


def _exclusion_csr_host(users, record):
    import torch
    if torch.is_tensor(users):
        users = users.cpu().numpy()
    users = np.asarray(users).reshape(-1)
    rows = [np.sort(np.fromiter(record.get(int(u), ()), dtype=np.int64)) for u in users]
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([r.size for r in rows])
    ids = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    return ptr, ids


# --------------------------------------------------------------------------- training loop
def train_epoch(args, model, train_data, user_triplet_set, sess=None, rng=None):
    """One epoch of train.py:56-64 through ``model.train(sess, feed_dict)``: shuffle, then full
    minibatches only (the ragged tail is skipped, train.py:60-62).  Returns the list of losses."""
    (rng or np.random).shuffle(train_data)
    losses, start = [], 0
    while start + args.batch_size <= train_data.shape[0]:
        _, loss = model.train(sess, get_feed_dict(args, model, train_data, user_triplet_set, start,
                                                  start + args.batch_size))
        losses.append(loss)
        start += args.batch_size
    return losses


def _epoch_trainer(feeder, batch_size, graph):
    """The model's Trainer (made on first use) and, for ``graph=True`` on one rank, its GraphedTrainer captured at
    ``batch_size`` (None: eager steps)."""
    from .training import GraphedTrainer, Trainer
    model = feeder.model
    if model.trainer is None:
        model.trainer = Trainer(model)
    gt = None
    if graph and model.trainer.world == 1:     # a data-parallel step keeps its all-reduce eager (GraphedTrainer refuses)
        gt = getattr(model, "_graphed_trainer", None)
        if (gt is None or gt.tr is not model.trainer or gt.users.shape[0] != batch_size
                or gt._storage_key() != gt._captured        # set_adjacency / a rebound parameter: capture again
                or gt.head != model.trainer.head_key()      # ... or another head (objective, group size, logit offset)
                or gt.guard != model.trainer.guard_key()):                                   # ... or the guard on / off
            try:
                gt = model._graphed_trainer = GraphedTrainer(model.trainer, batch_size)
            except RuntimeError as e:                       # capture failed: the same kernels, launched eagerly
                import warnings
                warnings.warn(f"hipGraph capture of the training step failed ({e}); running the epoch eagerly")
                gt = model._graphed_trainer = None
    return gt


def _run_epoch_on_device(feeder, data, batch_size, gt):
    """One epoch over ``data``, an int64 [n, 3] (user, item, label) tensor on the model's device, in row order: full
    minibatches only, the ragged tail dropped.  ``gt``: the GraphedTrainer of ``_epoch_trainer`` or None.  Returns the losses."""
    import torch
    model = feeder.model
    losses, start = [], 0
    while start + batch_size <= data.shape[0]:
        blk = data[start:start + batch_size]
        users, items, labels = blk[:, 0].contiguous(), blk[:, 1].contiguous(), blk[:, 2].to(torch.float32)
        mh, mr, mt = feeder.memories(users)
        if gt is not None:
            losses.append(gt.step(users, items, labels, mh, mr, mt).clone())
        else:
            losses.append(model.trainer.step(users, items, labels, mh, mr, mt))
        start += batch_size
    if gt is not None and losses:
        losses = torch.cat(losses).cpu().tolist()
    return losses


def train_epoch_device(feeder, train_data, batch_size, rng=None, graph=False):
    """Same epoch with device-side feeds (ripple sets gathered on the GPU).  ``graph=True``: every step is one
    hipGraph replay (training.GraphedTrainer, captured once per batch size) and the losses are read back once,
    at the end of the epoch, instead of once per step."""
    import torch
    gt = _epoch_trainer(feeder, batch_size, graph)
    (rng or np.random).shuffle(train_data)
    data = torch.from_numpy(np.ascontiguousarray(train_data)).to(feeder.model.device)
    return _run_epoch_on_device(feeder, data, batch_size, gt)


def _epoch_perm(sampler, round, n, device, perm_seed=None):
    """The permutation of an epoch's ``n`` rows or groups, on the device: a ``torch.Generator`` seeded with ``perm_seed``
    (None: derived from the sampler's seed and ``round``)."""
    import torch
    if perm_seed is None:
        perm_seed = (int(sampler.seed) * 0x9E3779B97F4A7C15 + int(round) * 0xC2B2AE3D27D4EB4F + 1) & ((1 << 63) - 1)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(perm_seed))
    return torch.randperm(n, generator=gen, device=device)


def resampled_epoch_rows(sampler, round, device, perm_seed=None):
    """The rows ``train_epoch_resampled`` trains on: ``sampler.epoch(round)`` permuted on the device by a
    ``torch.Generator`` seeded with ``perm_seed`` (None: derived from the sampler's seed and ``round``), so the same
    (sampler, round, perm_seed) gives the same rows in the same order.  int64 [n, 3] on ``device``; nothing goes to the host."""
    rows = sampler.epoch(round)
    return rows[_epoch_perm(sampler, round, rows.shape[0], device, perm_seed)]


def train_epoch_resampled(feeder, sampler, batch_size, round, graph=False, perm_seed=None):
    """One epoch whose label-0 rows are drawn for this epoch: the positives of ``sampler`` (data_prep.NegativeSampler) plus
    ``sampler.epoch(round)``'s fresh negatives, permuted on the device (``resampled_epoch_rows``), then full minibatches
    only through the same Trainer / GraphedTrainer steps as ``train_epoch_device``.  Returns the losses like it.
    The rows are a pure function of (sampler, round, perm_seed): every rank of a data-parallel run computes the same epoch
    tensor without communication, exactly as every rank holds the same ``train_data`` in ``train_epoch_device``."""
    gt = _epoch_trainer(feeder, batch_size, graph)
    data = resampled_epoch_rows(sampler, round, feeder.model.device, perm_seed)
    return _run_epoch_on_device(feeder, data, batch_size, gt)


def ranked_epoch_groups(sampler, round, device, perm_seed=None, logq=False):
    """The groups ``train_epoch_ranked`` trains on: ``data_prep.rank_groups(sampler, round)`` with the GROUPS permuted on the
    device, seeded exactly like ``resampled_epoch_rows``.  (users [n], items [n, G], valid [n, G]); nothing goes to the host.
    ``logq=True`` appends the epoch's logit offsets, f32 [n, G]: ``data_prep.rank_offsets`` of the permuted groups."""
    from .data_prep import rank_groups, rank_offsets
    users, items, valid = rank_groups(sampler, round)
    perm = _epoch_perm(sampler, round, users.shape[0], device, perm_seed)
    users, items, valid = users[perm], items[perm], valid[perm]
    if logq:
        return users, items, valid, rank_offsets(sampler, users, items, valid)
    return users, items, valid


def train_epoch_ranked(feeder, sampler, batch_size, round, objective, graph=False, perm_seed=None, logq=False):
    """One epoch under a ranking objective ("bpr" / "softmax", training.Trainer.set_objective): every positive of ``sampler``
    (a data_prep.NegativeSampler built with ``ratio`` = n_neg) against its n_neg fresh negatives of ``round``, as groups of
    G = 1 + n_neg rows.  The groups are permuted on the device (``ranked_epoch_groups``) and a step takes
    ``batch_size // G`` whole groups -- full steps only, the ragged tail dropped.  Returns the losses like the other epoch
    functions.  ``Trainer.rank_counts`` is zeroed at the start and read back ONCE at the end: the epoch's sampled pairwise
    accuracy (negatives scored below their positive, ties half) is left in ``model.trainer.last_pairwise_acc`` (nan for an
    epoch without a valid negative).  A pure function of (sampler, round, perm_seed), like ``train_epoch_resampled``.
    ``logq=True`` ("softmax" only): the logQ-corrected sampled softmax.  The epoch's logit offsets are built once from the
    permuted groups (``data_prep.rank_offsets``: log of a negative's expected sampling count under the sampler's proposal)
    and sliced per step like ``valid``; the head subtracts them before the softmax (mvin_rank_head_offset).  They are a pure
    function of (sampler, round, perm_seed) like the groups, so every rank of a data-parallel run builds the same ones.
    ``last_pairwise_acc`` keeps its meaning: it compares the raw scores."""
    import torch
    from .training import Trainer
    model = feeder.model
    G = 1 + int(sampler.ratio)
    n_g = int(batch_size) // G
    if n_g < 1:
        raise ValueError(f"batch_size={batch_size} holds no group of {G} rows")
    if model.trainer is None:
        model.trainer = Trainer(model)
    tr = model.trainer
    if logq and objective != "softmax":
        raise ValueError(f"logq=True corrects the sampled softmax: it needs objective='softmax', not {objective!r}")
    tr.set_objective(objective, G, offset=bool(logq))
    gt = _epoch_trainer(feeder, n_g * G, graph)
    users, items, valid, *offsets = ranked_epoch_groups(sampler, round, model.device, perm_seed, logq=bool(logq))
    tr.rank_counts.zero_()
    losses = _ranked_steps(feeder, tr, gt, users, items, valid, n_g, offsets=offsets[0] if logq else None)
    if gt is not None and losses:
        losses = torch.cat(losses).cpu().tolist()
    c0, c1 = tr.rank_counts.cpu().tolist()
    tr.last_pairwise_acc = c0 / (2.0 * c1) if c1 else float("nan")
    return losses


def _ranked_steps(feeder, tr, gt, users, items, valid, n_g, offsets=None):
    """The step loop of a ranked epoch (train_epoch_ranked, train_epoch_hard): ``n_g`` whole groups of ``users`` [n] /
    ``items`` / ``valid`` [n, G] (and ``offsets`` [n, G], the logit offsets of a logQ-corrected epoch, or None) per step, full
    steps only.  Returns the step losses: floats of the eager step (``gt`` None), device tensors of the replayed one (the
    caller reads them back once)."""
    G = items.shape[1]
    losses, start = [], 0
    while start + n_g <= users.shape[0]:
        u = users[start:start + n_g].repeat_interleave(G)
        it = items[start:start + n_g].reshape(-1)
        v = valid[start:start + n_g].reshape(-1)
        mh, mr, mt = feeder.memories(u)
        okw = {} if offsets is None else {"offset": offsets[start:start + n_g].reshape(-1)}
        if gt is not None:
            losses.append(gt.step(u, it, v, mh, mr, mt, **okw).clone())
        else:
            losses.append(tr.step(u, it, v, mh, mr, mt, **okw))
        start += n_g
    return losses


def score_pool(feeder, users, items, max_pairs=524288, out=None):
    """The current model's sigmoid scores of every slot of the pool groups ``users`` [n] / ``items`` [n, Gp] as one f32
    [n, Gp] device buffer (``out`` if given): ``DeviceFeeder.scores`` -- no gradient, no tape -- over chunks of whole groups of
    at most ``max_pairs`` pairs.  Enqueues only."""
    import torch
    n, Gp = items.shape
    per = max(1, int(max_pairs) // Gp)
    if out is None:
        out = torch.empty((n, Gp), dtype=torch.float32, device=items.device)
    for g0 in range(0, n, per):
        g1 = min(n, g0 + per)
        out[g0:g1].view(-1).copy_(feeder.scores(users[g0:g1].repeat_interleave(Gp), items[g0:g1].reshape(-1)))
    return out


def hard_epoch_groups(feeder, sampler, round, n_neg, shortlist, pool=None, index=None, counts=None, max_pairs=524288,
                      return_pool=False):
    """The groups ``train_epoch_hard`` trains on, for the weights the model has NOW: draw the pool
    (``data_prep.rank_groups(sampler, round)``, ``sampler`` built with ``ratio`` = the pool size M; or take ``pool``, that
    triple, from the caller), score every pool slot (``score_pool``), and let mvin_select_negatives pick ``n_neg`` of the
    ``shortlist`` highest-scored candidates of every group (``data_prep.hard_groups``).  ``index`` int64 [m]: the rows (in
    ``train_data`` order) to do this for, in that order -- a part of a permuted epoch; it is also each row's selection key, so
    a row's draw depends neither on the permutation nor on how the epoch is cut into parts.  None: every row.
    Returns (users [m], items [m, 1 + n_neg], valid [m, 1 + n_neg]); with ``return_pool`` also (pool items [m, 1 + M],
    pool valid, scores f32 [m, 1 + M]) of the same rows.  ``counts`` int64 [4] accumulates.  Nothing goes to the host."""
    from .data_prep import hard_groups, rank_groups
    users, items, valid = rank_groups(sampler, round) if pool is None else pool
    if index is not None:
        users, items, valid = users[index], items[index].contiguous(), valid[index].contiguous()
    scores = score_pool(feeder, users, items, max_pairs)
    out = hard_groups(sampler, round, scores, n_neg, shortlist, group_key=index, counts=counts, pool=(users, items, valid))
    return out + (items, valid, scores) if return_pool else out


def train_epoch_hard(feeder, sampler, batch_size, round, objective, n_neg, shortlist=None, rescore=1, graph=False,
                     perm_seed=None, max_pairs=524288):
    """One epoch under a ranking objective on HARD negatives (dynamic negative sampling): ``sampler`` is a
    data_prep.NegativeSampler built with ``ratio`` = the pool size M (n_neg <= M <= 63).  Every positive gets a pool of M
    distinct unwatched items of its user for ``round``; the pool is scored with the current weights and ``n_neg`` of the
    ``shortlist`` (None: n_neg, "the hardest") highest-scored candidates are trained on (``hard_epoch_groups``).  The groups are
    permuted and stepped through exactly as in ``train_epoch_ranked`` (same ``perm_seed`` rule, ``batch_size // (1 + n_neg)``
    whole groups per step, full steps only).  ``rescore`` = k cuts the permuted epoch into k consecutive parts and scores and
    selects each part immediately before training on it, so later parts see newer weights.  Single rank only: the ranks of a
    data-parallel run would have to reproduce the same scores bit for bit.
    Leaves in ``model.trainer``: ``last_pairwise_acc`` as ``train_epoch_ranked`` does, and ``last_hard_rate`` /
    ``last_pool_rate``, the share of the trained negatives / of all pool candidates that the model scored above their positive
    (ties half; nan without a candidate), exact integers read back once together with ``rank_counts``."""
    import torch
    from .data_prep import rank_groups
    from .training import Trainer
    model = feeder.model
    n_neg = int(n_neg)
    shortlist = n_neg if shortlist is None else int(shortlist)
    rescore = int(rescore)
    if rescore < 1:
        raise ValueError(f"rescore={rescore}: expected >= 1")
    G = 1 + n_neg
    n_g = int(batch_size) // G
    if n_g < 1:
        raise ValueError(f"batch_size={batch_size} holds no group of {G} rows")
    if model.trainer is None:
        model.trainer = Trainer(model)
    tr = model.trainer
    if tr.world > 1:
        raise ValueError(f"train_epoch_hard: single rank only (world={tr.world})")
    tr.set_objective(objective, G)
    gt = _epoch_trainer(feeder, n_g * G, graph)
    dev = model.device
    pool = rank_groups(sampler, round)
    n = pool[0].shape[0]
    perm = _epoch_perm(sampler, round, n, dev, perm_seed)
    tr.rank_counts.zero_()
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    steps = n // n_g
    losses = []
    for part in range(rescore):                  # parts of whole steps; the ragged tail is dropped as in train_epoch_ranked
        s0, s1 = steps * part // rescore, steps * (part + 1) // rescore
        if s1 == s0:
            continue
        users, items, valid = hard_epoch_groups(feeder, sampler, round, n_neg, shortlist, pool=pool,
                                                index=perm[s0 * n_g:s1 * n_g], counts=counts, max_pairs=max_pairs)
        losses += _ranked_steps(feeder, tr, gt, users, items, valid, n_g)
    if gt is not None and losses:
        losses = torch.cat(losses).cpu().tolist()
    c = torch.cat([tr.rank_counts, counts]).cpu().tolist()
    tr.last_pairwise_acc = c[0] / (2.0 * c[1]) if c[1] else float("nan")
    tr.last_hard_rate = c[2] / (2.0 * c[3]) if c[3] else float("nan")
    tr.last_pool_rate = c[4] / (2.0 * c[5]) if c[5] else float("nan")
    return losses


# --------------------------------------------------------------------------- ranking metrics
def precision_at_k(ranked, answers, k):
    """metrics.py:33-48: |top-k intersect answers| / k."""
    return len(set(ranked[:k]) & set(answers)) / k


def recall_at_k(ranked, answers, k):
    """metrics.py:96-111: |top-k intersect answers| / |answers|."""
    return len(set(ranked[:k]) & set(answers)) / len(answers)


def dcg_at_k(r, k):
    """metrics.py:3-18 with method=1: sum_i r_i / log2(i + 2)."""
    r = np.asarray(r, dtype=np.float64)[:k]
    return float(np.sum(r / np.log2(np.arange(2, r.size + 2)))) if r.size else 0.0


def ndcg_at_k(r, k):
    """metrics.py:21-31."""
    best = dcg_at_k(sorted(r, reverse=True), k)
    return dcg_at_k(r, k) / best if best else 0.0


# --------------------------------------------------------------------------- evaluations
def ctr_eval(args, model, data, user_triplet_set, batch_size, sess=None):
    """util.py:44-56 through the reference-shaped ``model.eval(sess, feed_dict)``."""
    aucs, accs, f1s = [], [], []
    start = 0
    while start + batch_size <= data.shape[0]:
        auc, acc, f1 = model.eval(sess, get_feed_dict(args, model, data, user_triplet_set, start, start + batch_size))
        aucs.append(auc)
        accs.append(acc)
        f1s.append(f1)
        start += batch_size
    return aucs, accs, f1s, float(np.mean(aucs)), float(np.mean(accs)), float(np.mean(f1s))


def eval_streams(model, batch_size):
    """How many HIP streams the independent batches of an evaluation go round-robin to (measured at C3): TWO where a pass is the
    single launch (<= MVIN.small_max_batch pairs: 24.3 us per 512-pair batch against 36.0 on one stream and 28.8 on three), THREE
    for the multi-launch schedule (4 096 pairs: 71 vs 76 us on two; 524 288: 1.058 vs 1.082 ms; four: 1.097)."""
    return 2 if batch_size <= int(getattr(model, "small_max_batch", 0) or 0) else 3


def ctr_eval_device(feeder, data, batch_size, streams=None, window=16):
    """Same numbers as ctr_eval, feeds assembled on the device.  The batches of an evaluation are independent: they are
    enqueued round-robin on ``streams`` HIP streams (None: ``eval_streams`` -- at the reference's batch sizes a scoring pass is one
    launch that walks a dependent chain of loads, two passes in flight overlap their waits: 24 vs 36 us per 512-pair batch at C3),
    ``window`` batches ahead of the host-side metrics; ``streams=1`` scores and reads back one batch at a time."""
    import torch
    from sklearn.metrics import f1_score, roc_auc_score
    aucs, accs, f1s = [], [], []
    starts = list(range(0, data.shape[0] - batch_size + 1, batch_size))
    dev = feeder.model.device
    from .graph import scoring_streams
    if streams is None:
        streams = eval_streams(feeder.model, batch_size)
    lanes = scoring_streams(dev, streams) if streams > 1 else None
    if lanes:
        # everything the forward builds lazily and CACHES (relation-logit tables dropped by invalidate() after a training epoch,
        # the adjacency encoding, the one-time id check and the static per-user records of user_triplet_set) is built here, on
        # the current stream, before the lanes start: a table built by the first batch on lane 0 would be read by the second
        # batch on lane 1 with nothing ordering the two
        feeder.model.prepare(getattr(feeder, "uts", None))
        for ln in lanes:
            ln.wait_stream(torch.cuda.current_stream(dev))
    pending = []

    def finish(entry):
        blk, s, ev = entry
        if ev is not None:
            ev.synchronize()
        s = s.cpu().numpy()
        labels = blk[:, 2].astype(np.float32)
        aucs.append(roc_auc_score(y_true=labels, y_score=s))
        pred = (s >= 0.5).astype(np.float32)
        f1s.append(f1_score(y_true=labels, y_pred=pred))
        accs.append(float(np.mean(pred == labels)))

    for i, start in enumerate(starts):
        blk = data[start:start + batch_size]
        if lanes:
            with torch.cuda.stream(lanes[i % streams]):
                s = feeder.scores(blk[:, 0], blk[:, 1])
                ev = torch.cuda.Event()
                ev.record()
        else:
            s, ev = feeder.scores(blk[:, 0], blk[:, 1]), None
        pending.append((blk, s, ev))
        if len(pending) > (window if lanes else 0):
            finish(pending.pop(0))
    while pending:
        finish(pending.pop(0))
    return aucs, accs, f1s, float(np.mean(aucs)), float(np.mean(accs)), float(np.mean(f1s))


def topk_settings(train_data, eval_data, test_data, n_item, user_num=250, k_list=(1, 2, 5, 10, 25, 50, 100)):
    """util.py:14-41 without the pickle round trip: the ``user_num`` users with the most
    positive train interactions among those present in all three splits."""
    train_record = get_user_record(train_data, True)
    test_record = get_user_record(test_data, False)
    eval_record = get_user_record(eval_data, False)
    users = list(set(train_record) & set(test_record) & set(eval_record))
    users = sorted(users, key=lambda u: len(train_record[u]), reverse=True)[:user_num]
    return users, train_record, eval_record, test_record, set(range(n_item)), list(k_list)


def _rank_metrics(item_sorted, truth, k_list, precision_list, recall_list, ndcg_list):
    for k in k_list:
        precision_list[k].append(precision_at_k(item_sorted, truth, k))
        recall_list[k].append(recall_at_k(item_sorted, truth, k))
    k_stale = k_list[-1]  # util.py:193 uses the loop variable left over from the loop above
    r_hit = [1 if i in truth else 0 for i in item_sorted[:k_stale]]
    for k in k_list:
        ndcg_list[k].append(ndcg_at_k(r_hit, k))


def topk_eval(args, user_triplet_set, model, user_list, train_record, eval_record, test_record, item_set,
              k_list, batch_size, mode="test", sess=None):
    """util.py:137-205 through ``model.get_scores(sess, feed_dict)``."""
    precision_list = {k: [] for k in k_list}
    recall_list = {k: [] for k in k_list}
    ndcg_list = {k: [] for k in k_list}
    ref = eval_record if mode == "eval" else test_record
    for user in user_list:
        if user not in ref:
            continue
        test_items = list(item_set - train_record[user])
        score_of = {}
        start = 0
        while start + batch_size <= len(test_items):
            items, scores = model.get_scores(sess, get_feed_dict_top_k(
                args, model, [user] * batch_size, test_items[start:start + batch_size], [1] * batch_size,
                user_triplet_set))
            score_of.update(zip(items, scores))
            start += batch_size
        if start < len(test_items):  # pad the ragged tail with its last item (util.py:166-177)
            pad = test_items[start:] + [test_items[-1]] * (batch_size - len(test_items) + start)
            items, scores = model.get_scores(sess, get_feed_dict_top_k(
                args, model, [user] * batch_size, pad, [1] * batch_size, user_triplet_set))
            score_of.update(zip(items, scores))
        item_sorted = [i for i, _ in sorted(score_of.items(), key=lambda x: x[1], reverse=True)]
        _rank_metrics(item_sorted, ref[user], k_list, precision_list, recall_list, ndcg_list)
    return ([float(np.mean(precision_list[k])) for k in k_list], [float(np.mean(recall_list[k])) for k in k_list],
            [float(np.mean(ndcg_list[k])) for k in k_list], None, None)


def topk_eval_device(feeder, user_list, train_record, eval_record, test_record, item_set, k_list,
                     batch_size, mode="test"):
    """top-K evaluation with device-side feeds.  Every (user, candidate item) pair is scored
    exactly once (no padded duplicates: the scoring path takes any batch length); ranking
    ties are broken like the reference's ``sorted`` (stable, by insertion order)."""
    precision_list = {k: [] for k in k_list}
    recall_list = {k: [] for k in k_list}
    ndcg_list = {k: [] for k in k_list}
    ref = eval_record if mode == "eval" else test_record
    for user in user_list:
        if user not in ref:
            continue
        test_items = np.fromiter(item_set - train_record[user], dtype=np.int64)
        scores = np.empty(len(test_items), dtype=np.float32)
        for start in range(0, len(test_items), batch_size):
            blk = test_items[start:start + batch_size]
            scores[start:start + len(blk)] = feeder.scores_user(user, blk).cpu().numpy()
        order = np.argsort(-scores, kind="stable")
        _rank_metrics(test_items[order].tolist(), ref[user], k_list, precision_list, recall_list, ndcg_list)
    return ([float(np.mean(precision_list[k])) for k in k_list], [float(np.mean(recall_list[k])) for k in k_list],
            [float(np.mean(ndcg_list[k])) for k in k_list], None, None)


def topk_eval_batched(feeder, user_list, train_record, eval_record, test_record, item_set, k_list, mode="test",
                      max_pairs=524288):
    """topk_eval_device's numbers from ONE batched recommendation: the users of ``user_list`` present in the ``mode`` record are
    scored against ``sorted(item_set)`` and ranked on the device (DeviceFeeder.recommend, mvin_topk_rows), their train items
    excluded; one copy of the [U, max(k_list)] ids comes back.  The top max(k_list) items are all the metrics read, the stale-k
    NDCG list included (k_list[-1] <= max(k_list)).  Ties go to the lower item id (topk_eval_device inherits the set's
    iteration order, which is usually but not always ascending)."""
    precision_list = {k: [] for k in k_list}
    recall_list = {k: [] for k in k_list}
    ndcg_list = {k: [] for k in k_list}
    ref = eval_record if mode == "eval" else test_record
    users = [u for u in user_list if u in ref]
    if users:
        items, _ = feeder.recommend(users, max(k_list), sorted(item_set), exclude=train_record, max_pairs=max_pairs)
        items = items.cpu().numpy()
        for user, row in zip(users, items):
            _rank_metrics(row[row >= 0].tolist(), ref[user], k_list, precision_list, recall_list, ndcg_list)
    return ([float(np.mean(precision_list[k])) for k in k_list], [float(np.mean(recall_list[k])) for k in k_list],
            [float(np.mean(ndcg_list[k])) for k in k_list], None, None)


def diversity_eval(feeder, users, lists, truth_record, k, lams=(1.0, 0.7, 0.5, 0.3), exclude=None, n_item=None, features=None,
                   cosine=True, max_pairs=524288):
    """What the relevance / redundancy trade-off of DeviceFeeder.diversify_lists costs and buys on given candidate lists: ONE
    ``diversify_lists`` call and ONE copy back (items, penalties and similarity sums packed into one int32 tensor) per ``lam``
    of ``lams``, the rest in float64 on the host.  ``users`` on the host; ``lists``, ``exclude``, ``features``, ``cosine`` and
    ``max_pairs`` as in ``diversify_lists``; ``truth_record``: a get_user_record dict of held-out items.  Returns one dict per
    ``lam``, in order:
      lam; recall, ndcg -- recall_at_k and ndcg_at_k (hits in the returned order) at ``k``, means over the ``n_users`` users
      with a non-empty ``truth_record`` entry (0.0 without such a user);
      ild -- intra-list diversity, 1 - (sum of a list's simsums) / (m (m - 1) / 2) over its m picks, the mean over the
      ``n_lists`` lists with m >= 2 (NaN without one);
      coverage -- the distinct items over all returned lists / ``n_item`` (None: the rows of the feature table);
      penalty -- the mean penalty over the filled slots after each list's first (NaN without one);
      items -- the returned lists, int64 [U, k] on the host (-1 = padding): the ``lam = 1.0`` row carries ``recommend_lists``'."""
    import torch
    k = int(k)
    if k < 1:
        raise ValueError(f"diversity_eval: k={k}")
    lams = [float(x) for x in lams]
    if not lams or any(not 0.0 <= x <= 1.0 for x in lams):
        raise ValueError(f"diversity_eval: lams={lams}: expected at least one value, each in [0, 1]")
    if not isinstance(truth_record, dict):
        raise ValueError("diversity_eval: truth_record must be a dict of user -> held-out items")
    if torch.is_tensor(users) and users.is_cuda:
        raise ValueError("diversity_eval: users must be on the host (they index truth_record)")
    users = np.asarray(users.numpy() if torch.is_tensor(users) else users, dtype=np.int64).reshape(-1)
    U = users.size
    if n_item is None:
        n_item = int((feeder.model.entity_emb_matrix if features is None else features).shape[0])
    if int(n_item) < 1:
        raise ValueError(f"diversity_eval: n_item={n_item}")
    rows = []
    for lam in lams:
        items, _, _, pen, simsum = feeder.diversify_lists(users, lists, k, lam=lam, features=features, cosine=cosine, exclude=exclude,
                                                          max_pairs=max_pairs)
        packed = torch.cat([items.to(torch.int32).reshape(-1), pen.reshape(-1).view(torch.int32),
                            simsum.reshape(-1).view(torch.int32)]).cpu().numpy()
        n = U * k
        it = packed[:n].reshape(U, k).astype(np.int64)
        pn = packed[n:2 * n].view(np.float32).reshape(U, k).astype(np.float64)
        ss = packed[2 * n:].view(np.float32).reshape(U, k).astype(np.float64)
        recall, ndcg, ild, pens = [], [], [], []
        for i, user in enumerate(users):
            m = int((it[i] >= 0).sum())
            ranked = it[i][:m].tolist()
            truth = truth_record.get(int(user))
            if truth:
                recall.append(recall_at_k(ranked, truth, k))
                ndcg.append(ndcg_at_k([1 if x in truth else 0 for x in ranked], k))
            if m >= 2:
                ild.append(1.0 - float(ss[i][:m].sum()) / (m * (m - 1) / 2.0))
                pens.extend(pn[i][1:m].tolist())
        rows.append(dict(lam=lam, recall=float(np.mean(recall)) if recall else 0.0, ndcg=float(np.mean(ndcg)) if ndcg else 0.0,
                         ild=float(np.mean(ild)) if ild else float("nan"), coverage=len(set(it[it >= 0].tolist())) / float(n_item),
                         penalty=float(np.mean(pens)) if pens else float("nan"), n_users=len(recall), n_lists=len(ild), items=it))
    return rows


def retrieval_eval(feeder, users, train_record, truth_record, candidates, n_cand_list, k, history, full_users=0, cosine=False,
                   max_pairs=524288, retriever=None):
    """What first-stage retrieval with the history-mean query (DeviceFeeder.user_queries, a PROXY for MVIN's item-dependent
    user vector) keeps of the model's ranking: for every ``n_cand`` of ``n_cand_list`` ONE ``retrieve`` (the user's
    ``train_record`` items excluded), ONE ``recommend_lists`` over the retrieved lists and ONE copy back (both id matrices
    packed into one int32 tensor), the rest in float64 on the host.  ``users`` on the host; only those with a non-empty
    ``truth_record`` entry (a get_user_record dict of held-out items) are taken.  Returns one dict per ``n_cand``, in order:
      n_cand; candidate_recall -- the share of a user's held-out items that reach the retrieved list, the mean over users;
      recall, ndcg -- recall_at_k and ndcg_at_k (hits in the returned order) at ``k`` of the two-stage result, means over users;
      overlap -- with ``full_users`` > 0: |two-stage top-k intersect ``recommend``'s top-k| / |``recommend``'s top-k| over
      the first ``full_users`` users (``recommend`` over all candidates runs once, one more copy back), else None;
      n_users; items -- the two-stage lists, int64 [U, k] on the host (-1 = padding).
    ``retriever`` (None: the proxy above): an object with ``retrieve(users, n_cand, candidates, exclude=...)``, e.g. an
    ``mf.MFFeeder``; its lists are the first stage (``history`` and ``cosine`` are then not used) and the report is the same, so
    the proxy and a learned tower are compared on candidate recall and overlap."""
    import torch
    k = int(k)
    if k < 1:
        raise ValueError(f"retrieval_eval: k={k}")
    n_cand_list = [int(x) for x in n_cand_list]
    if not n_cand_list or any(not 1 <= x <= 1024 for x in n_cand_list):
        raise ValueError(f"retrieval_eval: n_cand_list={n_cand_list}: expected at least one value, each in 1 .. 1024")
    if not isinstance(truth_record, dict) or not isinstance(train_record, dict):
        raise ValueError("retrieval_eval: train_record and truth_record must be dicts of user -> items")
    if torch.is_tensor(users) and users.is_cuda:
        raise ValueError("retrieval_eval: users must be on the host (they index the records)")
    users = [int(x) for x in np.asarray(users.numpy() if torch.is_tensor(users) else users, dtype=np.int64).reshape(-1)
             if truth_record.get(int(x))]
    U, F = len(users), min(int(full_users), len(users))
    excl = feeder.exclusion_csr(users, train_record)
    full = None
    if F > 0:
        full_ids, _ = feeder.recommend(users[:F], k, candidates, exclude=(excl[0][:F + 1], excl[1]))
        full = full_ids.to(torch.int32).cpu().numpy().reshape(F, k)
    rows = []
    for n_cand in n_cand_list:
        if retriever is not None:
            cand, _ = retriever.retrieve(users, n_cand, candidates, exclude=excl)
        else:
            cand, _ = feeder.retrieve(users, n_cand, candidates, history=history, cosine=cosine, exclude=excl)
        ptr = np.arange(U + 1, dtype=np.int64) * n_cand
        top, _, _ = feeder.recommend_lists(users, (ptr, cand.reshape(-1)), k, max_pairs=max_pairs)
        packed = torch.cat([cand.to(torch.int32).reshape(-1), top.to(torch.int32).reshape(-1)]).cpu().numpy()
        cd = packed[:U * n_cand].reshape(U, n_cand).astype(np.int64)
        it = packed[U * n_cand:].reshape(U, k).astype(np.int64)
        cr, recall, ndcg, overlap = [], [], [], []
        for i, user in enumerate(users):
            truth = set(int(x) for x in truth_record[user])
            ranked = [int(x) for x in it[i] if x >= 0]
            cr.append(len(truth & set(int(x) for x in cd[i] if x >= 0)) / float(len(truth)))
            recall.append(recall_at_k(ranked, truth, k))
            ndcg.append(ndcg_at_k([1 if x in truth else 0 for x in ranked], k))
            if i < F:
                ref = set(int(x) for x in full[i] if x >= 0)
                overlap.append(len(ref & set(ranked)) / float(len(ref)) if ref else 1.0)
        rows.append(dict(n_cand=n_cand, candidate_recall=float(np.mean(cr)) if cr else 0.0,
                         recall=float(np.mean(recall)) if recall else 0.0, ndcg=float(np.mean(ndcg)) if ndcg else 0.0,
                         overlap=float(np.mean(overlap)) if overlap else None, n_users=U, items=it))
    return rows


def _ranked_metrics(feeder, users, positives, exclude, candidates, k_list, ndcg_window, max_pairs, auc=True):
    """rank_positives for ``users`` and ONE copy back (counts, value bits and eligible counts packed into one int32 tensor):
    the per-user arrays of ops.rank_metrics_from_counts."""
    import torch
    from . import ops
    ptr, ids = _exclusion_csr_host(users, positives)
    dev = feeder.model.device
    pos = (torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev))
    _, _, counts, vals, eligible = feeder.rank_positives(users, pos, candidates, exclude=exclude, max_pairs=max_pairs)
    T, U = ids.size, len(users)
    packed = torch.cat([counts.reshape(-1), vals.view(torch.int32), eligible]).cpu().numpy()
    return ops.rank_metrics_from_counts(ptr, packed[:3 * T].reshape(T, 3), packed[4 * T:4 * T + U], k_list,
                                        vals=packed[3 * T:4 * T].view(np.float32) if auc else None, ndcg_window=ndcg_window)


def rank_eval_per_user(feeder, users, train_record, truth_record, item_set, k_list, max_pairs=524288, ndcg_window=None):
    """rank_eval's per-user values, kept: ``{"users": [...], "k_list": [...], metric: f64 [U, len(k_list)] for every metric of
    ops.RANK_METRICS, "auc": f64 [U]}`` for the ``users`` present in ``truth_record``, in their order (NaN where a metric is not
    defined for a user).  What metric_intervals and compare_rankings resample."""
    from . import ops
    users = [u for u in users if u in truth_record]
    ks = [int(k) for k in k_list]
    if not users:
        per = {m: np.zeros((0, len(ks)), dtype=np.float64) for m in ops.RANK_METRICS}
        per["auc"] = np.zeros(0, dtype=np.float64)
    else:
        per = dict(_ranked_metrics(feeder, users, truth_record, train_record, sorted(item_set), ks, ndcg_window, max_pairs))
    per["users"], per["k_list"] = list(users), ks
    return per


def _per_user_table(per):
    """The metric columns of a rank_eval_per_user dict side by side, f64 [U, 7 len(k) + 1]: metric-major, k-minor, auc last."""
    from . import ops
    nk = len(per["k_list"])
    cols = [np.asarray(per[m], dtype=np.float64).reshape(-1, nk) for m in ops.RANK_METRICS]
    return np.concatenate(cols + [np.asarray(per["auc"], dtype=np.float64).reshape(-1, 1)], axis=1)


def _split_columns(flat, nk):
    """A [7 nk + 1] vector back as {metric: list per k, "auc": float}."""
    from . import ops
    out = {m: [float(v) for v in flat[i * nk:(i + 1) * nk]] for i, m in enumerate(ops.RANK_METRICS)}
    out["auc"] = float(flat[len(ops.RANK_METRICS) * nk])
    return out


def metric_intervals(per, level=0.95, n_rep=2000, seed=1, device="cuda"):
    """Percentile bootstrap intervals (users resampled with replacement, ``n_rep`` replicates of ``seed``) of every metric of a
    rank_eval_per_user dict: ONE upload of the f64 [U, 7 len(k) + 1] table, one "observed" and one "bootstrap" call of
    ops.resample_sums (mvin_resample_sums), ONE copy back, ops.resample_summary on the host.  Returns ``{metric: {"mean", "se",
    "lo", "hi"}}`` with a list per k (a float each for ``auc``) and ``n_users``.  ``mean`` is the column's sum in the kernel's
    summation order over its count: rank_eval's mean up to the f64 summation order -- rank_eval's own mean stays the reported
    number, this one only says where the interval sits.  All columns share one draw of users per replicate."""
    import torch
    from . import ops
    nk = len(per["k_list"])
    tab = _per_user_table(per)
    U, M = tab.shape
    t = torch.from_numpy(np.ascontiguousarray(tab)).to(device)
    o_s, o_c = ops.resample_sums(t, 1, seed=seed, mode="observed")
    b_s, b_c = ops.resample_sums(t, n_rep, seed=seed, mode="bootstrap")
    R = int(n_rep)
    (o_s, b_s), (o_c, b_c) = _copy_back([o_s, b_s], [o_c, b_c])
    summ = ops.resample_summary(o_s.reshape(-1), o_c.reshape(-1), b_s, b_c, level=level)
    parts = {key: _split_columns(summ[key], nk) for key in ("mean", "se", "lo", "hi")}
    out = {m: {key: parts[key][m] for key in parts} for m in list(ops.RANK_METRICS) + ["auc"]}
    out["n_users"] = U
    return out


def _add_intervals(out, per, ci, n_rep, ci_seed, device):
    """rank_eval's ``ci`` and ``se`` entries from metric_intervals."""
    from . import ops
    iv = metric_intervals(per, level=ci, n_rep=n_rep, seed=ci_seed, device=device)
    out["ci"] = {m: list(zip(iv[m]["lo"], iv[m]["hi"])) for m in ops.RANK_METRICS}
    out["ci"]["auc"] = (iv["auc"]["lo"], iv["auc"]["hi"])
    out["se"] = {m: iv[m]["se"] for m in ops.RANK_METRICS}
    out["se"]["auc"] = iv["auc"]["se"]


def rank_eval(feeder, users, train_record, truth_record, item_set, k_list, max_pairs=524288, ndcg_window=None, ci=None, n_rep=2000,
              ci_seed=1):
    """Ranking metrics of the ``users`` present in ``truth_record`` from the exact ranks of their truth items among
    ``sorted(item_set)``, their ``train_record`` items excluded (DeviceFeeder.rank_positives, mvin_rank_positives): no top-K
    selection, so no bound on k, and one copy of a few ints per truth item comes back.  Returns a dict of means over those
    users: a list per k of ``k_list`` for precision, recall, hit_ratio, mrr, map, ndcg (window ``ndcg_window``, default
    max(k_list)) and ndcg_ideal as ops.rank_metrics_from_counts defines them, ``auc`` (the mean of the per-user AUC of truth
    items against the other eligible candidates, over the users where it is defined) and ``n_users``.
    ``ci`` (a level such as 0.95; None: the dict and the launches above, nothing more) adds ``"ci"``: metric -> a list of
    ``(lo, hi)`` per k, and ``auc`` -> ``(lo, hi)``, the percentile bootstrap interval over users of metric_intervals (``n_rep``
    replicates of ``ci_seed``), and ``"se"``: the bootstrap standard errors in the same layout."""
    import warnings
    from . import ops
    per = rank_eval_per_user(feeder, users, train_record, truth_record, item_set, k_list, max_pairs=max_pairs, ndcg_window=ndcg_window)
    users = per["users"]
    out = {m: [float("nan")] * len(k_list) for m in ops.RANK_METRICS}
    out.update(auc=float("nan"), n_users=len(users))
    if not users:
        return out
    for m in ops.RANK_METRICS:
        out[m] = [float(np.mean(per[m][:, q].tolist())) for q in range(len(k_list))]
    defined = per["auc"][~np.isnan(per["auc"])]
    out["auc"] = float(np.mean(defined)) if defined.size else float("nan")
    if ci is not None:
        _add_intervals(out, per, ci, n_rep, ci_seed, feeder.model.device)
    return out


def compare_rankings(per_a, per_b, level=0.95, n_rep=10000, seed=1, device="cuda"):
    """Paired comparison of two rank_eval_per_user dicts over the SAME users (equal ``users`` lists and ``k_list``, else
    ValueError naming the first difference).  The difference columns d = a - b are formed on the host in f64 (NaN where either
    is NaN), ONE table [a | b | d] is uploaded, and ops.resample_sums runs "observed", "bootstrap" and "signflip" over it: every
    replicate resamples a, b and d with the same users.  Returns ``{metric: {...}, "auc": {...}, "n_users", "k_list", "n_rep"}``;
    per metric, a list per k (a float each for ``auc``) of ``mean_a``, ``mean_b`` (over the users where each is defined),
    ``diff`` (the mean of d over the users where both are), ``diff_lo`` / ``diff_hi`` (the percentile bootstrap interval of that
    mean at ``level``), ``p`` (the two-sided sign-flip permutation p-value of sum d, ops.signflip_pvalue; NaN where d has no
    defined user) and ``p_holm`` (Holm-adjusted over all metric x k cells of the call, auc included)."""
    import torch
    from . import ops
    ua, ub = list(per_a["users"]), list(per_b["users"])
    if len(ua) != len(ub):
        raise ValueError(f"compare_rankings: {len(ua)} users against {len(ub)}: the two evaluations must cover the same users")
    for i, (x, y) in enumerate(zip(ua, ub)):
        if x != y:
            raise ValueError(f"compare_rankings: users differ first at position {i}: {x} against {y}")
    if list(per_a["k_list"]) != list(per_b["k_list"]):
        raise ValueError(f"compare_rankings: k_list {list(per_a['k_list'])} against {list(per_b['k_list'])}")
    nk = len(per_a["k_list"])
    a, b = _per_user_table(per_a), _per_user_table(per_b)
    U, M = a.shape
    tab = np.ascontiguousarray(np.concatenate([a, b, a - b], axis=1))            # NaN - x = NaN
    t = torch.from_numpy(tab).to(device)
    R = int(n_rep)
    o_s, o_c = ops.resample_sums(t, 1, seed=seed, mode="observed")
    b_s, b_c = ops.resample_sums(t, R, seed=seed, mode="bootstrap")
    f_s, _ = ops.resample_sums(t[:, 2 * M:], R, seed=seed, mode="signflip")
    (o_s, b_s, f_s), (o_c, b_c) = _copy_back([o_s, b_s, f_s], [o_c, b_c])
    o_s, o_c = o_s.reshape(-1), o_c.reshape(-1)
    summ = ops.resample_summary(o_s, o_c, b_s, b_c, level=level)
    p = ops.signflip_pvalue(o_s[2 * M:], f_s)
    p = np.where(o_c[2 * M:] > 0, p, np.nan)
    cells = dict(mean_a=summ["mean"][:M], mean_b=summ["mean"][M:2 * M], diff=summ["mean"][2 * M:], diff_lo=summ["lo"][2 * M:],
                 diff_hi=summ["hi"][2 * M:], p=p, p_holm=ops.holm_adjust(p))
    parts = {key: _split_columns(v, nk) for key, v in cells.items()}
    out = {m: {key: parts[key][m] for key in parts} for m in list(ops.RANK_METRICS) + ["auc"]}
    out.update(n_users=U, k_list=list(per_a["k_list"]), n_rep=R)
    return out


def topk_eval_ranked(feeder, user_list, train_record, eval_record, test_record, item_set, k_list, mode="test",
                     max_pairs=524288):
    """topk_eval_batched's numbers, equal to the last bit, from ranks instead of a selection: the same users are scored against
    ``sorted(item_set)`` by the same calls, mvin_rank_positives finds the place of every truth item among the user's eligible
    candidates, and precision / recall / the stale-k NDCG follow from those places (ops.rank_metrics_from_counts with the
    window k_list[-1]).  No k is too large for it, and what comes back is a few ints per truth item."""
    ref = eval_record if mode == "eval" else test_record
    users = [u for u in user_list if u in ref]
    p, r, n = ([[] for _ in k_list] for _ in range(3))
    if users:
        per = _ranked_metrics(feeder, users, ref, train_record, sorted(item_set), k_list, k_list[-1], max_pairs, auc=False)
        p, r, n = ([per[m][:, q].tolist() for q in range(len(k_list))] for m in ("precision", "recall", "ndcg"))
    return ([float(np.mean(x)) for x in p], [float(np.mean(x)) for x in r], [float(np.mean(x)) for x in n], None, None)


def _full_ranking_protocol(train_data, split_data, users=None):
    """(users, train_record, truth) of the all-ranking protocol; ``users``: keep only these (those with a label-1 row)."""
    train_record = get_user_record(np.asarray(train_data), True)
    truth = get_user_record(np.asarray(split_data), False)
    truth = {int(u): v for u, v in truth.items()}
    keep = sorted(truth) if users is None else sorted({int(u) for u in users} & set(truth))
    return keep, {int(u): v for u, v in train_record.items()}, truth


def full_ranking_eval(feeder, train_data, split_data, n_item, k_list=(20, 40, 60, 80, 100), max_pairs=524288, ci=None, n_rep=2000,
                      ci_seed=1):
    """The all-ranking protocol of the KG-recommender papers (the reference's KGAT/utility/batch_test.py:test): EVERY user
    with a label-1 row in ``split_data`` against the whole catalogue ``range(n_item)``, the user's label-1 items of
    ``train_data`` masked, each metric averaged over those users.  Returns rank_eval's dict (ndcg over the window max(k_list),
    as that protocol computes it, and the per-user AUC; with ``ci`` its bootstrap intervals and standard errors)."""
    users, train_record, truth = _full_ranking_protocol(train_data, split_data)
    return rank_eval(feeder, users, train_record, truth, range(int(n_item)), list(k_list), max_pairs=max_pairs, ci=ci, n_rep=n_rep,
                     ci_seed=ci_seed)


def compare_models(feeder_a, feeder_b, train_data, split_data, n_item, k_list=(20, 40, 60, 80, 100), users=None, level=0.95,
                   n_rep=10000, seed=1, max_pairs=524288):
    """Is model A better than model B on this split?  full_ranking_eval's protocol for both feeders over the same users
    (``users``: restrict it to these -- a sample keeps the two full-catalogue passes short), then compare_rankings on the two
    sets of per-user values: per metric and k the two means, the mean difference with its paired bootstrap interval, the
    sign-flip p-value and its Holm adjustment over every cell of the call."""
    keep, train_record, truth = _full_ranking_protocol(train_data, split_data, users)
    per = [rank_eval_per_user(f, keep, train_record, truth, range(int(n_item)), list(k_list), max_pairs=max_pairs)
           for f in (feeder_a, feeder_b)]
    return compare_rankings(per[0], per[1], level=level, n_rep=n_rep, seed=seed, device=feeder_a.model.device)


def _sampled_summary(users, counts, vals, eligible, k_list):
    """The sampled-candidate metrics of groups with ONE query each (group i belongs to ``users[i]``), from rank_segments'
    integers on the host: every metric of ops.rank_metrics_from_counts and the AUC, averaged over the groups, and the same
    under "by_user": the mean over users of each user's mean over its groups (an undefined AUC is left out of both means)."""
    from . import ops
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    n = users.size
    out = {m: [float("nan")] * len(k_list) for m in ops.RANK_METRICS}
    out.update(auc=float("nan"), n_users=int(np.unique(users).size), n_groups=int(n))
    out["by_user"] = {m: [float("nan")] * len(k_list) for m in ops.RANK_METRICS}
    out["by_user"]["auc"] = float("nan")
    if n == 0:
        return out
    import warnings
    # a group's metrics depend on its three counts and its eligible count alone (one query: its value ties with no other
    # query), so each DISTINCT (counts, eligible) goes through rank_metrics_from_counts once: a few thousand rows, not one
    # per held-out interaction
    c = np.asarray(counts).astype(np.int64).reshape(n, 3) + 1                  # -1 (missing) .. 4 096 -> 13 bits each
    key = ((c[:, 0] << 39) | (c[:, 1] << 26) | (c[:, 2] << 13)) | (np.asarray(eligible).astype(np.int64).reshape(n) + 1)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ops.UndefinedMetricWarning)            # a group of one eligible entry has no AUC
        cls = ops.rank_metrics_from_counts(np.arange(first.size + 1), np.asarray(counts).reshape(n, 3)[first],
                                           np.asarray(eligible).reshape(n)[first], k_list,
                                           vals=np.asarray(vals, dtype=np.float32).reshape(n)[first])
    per = {m: v[inv] for m, v in cls.items()}
    _, inv = np.unique(users, return_inverse=True)
    n_of = np.bincount(inv).astype(np.float64)
    for m in ops.RANK_METRICS:
        out[m] = [float(np.mean(per[m][:, q])) for q in range(len(k_list))]
        out["by_user"][m] = [float(np.mean(np.bincount(inv, weights=per[m][:, q]) / n_of)) for q in range(len(k_list))]
    ok = ~np.isnan(per["auc"])
    if ok.any():
        out["auc"] = float(np.mean(per["auc"][ok]))
        have = np.bincount(inv[ok], minlength=n_of.size).astype(np.float64)
        tot = np.bincount(inv[ok], weights=per["auc"][ok], minlength=n_of.size)
        out["by_user"]["auc"] = float(np.mean(tot[have > 0] / have[have > 0]))
    return out


def sampled_rank_eval(feeder, train_data, split_data, other_splits, n_user, n_item, n_neg=99, k_list=(5, 10, 20), seed=1,
                      round=0, max_pairs=524288):
    """SAMPLED-candidate evaluation, the leave-one-out protocol of NCF (He et al. 2017): every label-1 row of ``split_data``
    is ranked against ``n_neg`` (1..4095) sampled items the user has with label 1 in none of ``train_data``, ``split_data``
    and ``other_splits`` (data_prep.candidate_groups over a NegativeSampler of the split: a pure function of (``seed``,
    ``round``), the positive at a drawn slot so that ties are not handed to it).  The groups are scored through
    ``forward_users`` and ranked by ops.rank_segments in chunks of whole groups of at most ``max_pairs`` pairs, and ONE packed
    copy comes back.  Returns rank_eval's dict with every metric averaged over the held-out interactions (``n_users`` = the
    distinct users among them), the same metrics under ``"by_user"`` (the mean over users of each user's mean), ``n_groups``
    and ``n_short`` (slots the sampler could not fill: id -1, never eligible).
    The metrics are SAMPLED: their values depend on ``n_neg`` and on the draw, they are systematically higher than -- and not
    comparable with -- those of full ranking (rank_eval, full_ranking_eval; Krichene & Rendle 2020), and serve to follow one
    model over its epochs at a fraction of full ranking's cost."""
    import torch
    from . import ops
    from .data_prep import NegativeSampler, candidate_groups
    import warnings
    dev = feeder.model.device
    n_neg, max_pairs = int(n_neg), int(max_pairs)
    if max_pairs < 1:
        raise ValueError(f"max_pairs={max_pairs}")
    split = np.asarray(split_data, dtype=np.int64).reshape(-1, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # a clipped user is reported through n_short, not warned about
        sampler = NegativeSampler(split, n_user, n_item, exclude=(np.asarray(train_data),) + tuple(np.asarray(o) for o in other_splits),
                                  ratio=float(n_neg), seed=seed, device=dev)
    users, items, ids, slot = candidate_groups(sampler, round, n_neg)
    users_host = split[split[:, 2] == 1, 0]
    n, G = int(users.shape[0]), 1 + n_neg
    distinct = int(np.unique(users_host).size)
    flat = torch.empty((n * G,), dtype=torch.float32, device=dev)
    seg_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * G
    q_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev)
    out = (torch.empty((n, 3), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev),
           torch.empty((n,), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
    ids_flat, items_flat = ids.reshape(-1), items.reshape(-1)
    per = max(1, max_pairs // G)
    for g0 in range(0, n, per):
        g1 = min(n, g0 + per)
        lo, u_exp = g0 * G, users[g0:g1].repeat_interleave(G)
        for a in range(lo, g1 * G, max_pairs):                 # one piece, unless a single group is larger than max_pairs
            b = min(g1 * G, a + max_pairs)
            flat[a:b] = feeder.model.forward_users(u_exp[a - lo:b - lo], items_flat[a:b], feeder.uts,
                                                   distinct_users=min(distinct, g1 - g0)).scores_normalized
        ops.rank_segments(flat, seg_ptr[g0:g1 + 1], (q_ptr[g0:g1 + 1], slot), ids=ids_flat, max_len=G,
                          out=(out[0], out[1], out[2][g0:g1], out[3]))
    n_short = (ids_flat < 0).sum().to(torch.int32).reshape(1)
    packed = torch.cat([out[0].reshape(-1), out[1].view(torch.int32), out[2], n_short]).cpu().numpy()
    res = _sampled_summary(users_host, packed[:3 * n].reshape(n, 3), packed[3 * n:4 * n].view(np.float32), packed[4 * n:5 * n],
                           list(k_list))
    res["n_short"] = int(packed[5 * n])
    return res


def topk_eval_sampled(feeder, train_data, eval_data, test_data, n_user, n_item, k_list, mode="test", n_neg=99, seed=1, round=0,
                      max_pairs=524288):
    """topk_eval_ranked's return shape from sampled-candidate evaluation (sampled_rank_eval) of the ``mode`` split: per k the
    precision, recall and ndcg averaged over the held-out interactions of that split, each ranked against ``n_neg`` sampled
    items.  With one truth item per group recall is the hit ratio.  SAMPLED numbers: not comparable with the other
    ``topk_eval_*`` functions' (see sampled_rank_eval)."""
    split, other = (eval_data, test_data) if mode == "eval" else (test_data, eval_data)
    res = sampled_rank_eval(feeder, train_data, split, (other,), n_user, n_item, n_neg=n_neg, k_list=k_list, seed=seed,
                            round=round, max_pairs=max_pairs)
    return res["precision"], res["recall"], res["ndcg"], None, None


# --------------------------------------------------------------------------- the train.py loop
class EarlyStop(object):
    """train_util.py:20-61 (Early_stop_info): keep the best evaluation score, save the stage-wise
    tables whenever it improves (``save_final_model``), stop after ``early_stop`` epochs without
    improvement once ``tolerance`` epochs have passed."""

    def __init__(self, tolerance=2, early_stop=3, save_final_model=True):
        self.best, self.best_saved = -float("inf"), -float("inf")
        self.counter, self.tolerance, self.early_stop = 0, tolerance, early_stop
        self.save_final_model = save_final_model
        self.on_best = None          # called as on_best(epoch, score, model) wherever the best-epoch save happens (train's ``on_best``)

    def update(self, epoch, score, model):
        if score > self.best_saved:
            self.best_saved = score
            if self.on_best is not None:
                self.on_best(epoch, score, model)
            if self.save_final_model and model.path is not None and getattr(model.path, "emb", None):
                model.save_pretrain_emb_fuc(None, None)
        if epoch + 1 > self.tolerance:
            if score > self.best:
                self.best, self.counter = score, 0
            else:
                self.counter += 1
            if self.counter >= self.early_stop:
                return True
        return False


def train(args, data, show_topk=False, model=None, device="cuda", rng=None, log=None, topk_batch=65536, hoist=True,
          topk_early_stop=False, graph="auto", topk_impl="host", ctr_impl="host", negatives="fixed", on_best=None,
          objective="bce", n_neg=1, pool=16, shortlist=None, rescore=1, neg_dist="uniform", neg_alpha=0.75, neg_smooth=0.0,
          clip_norm=None, skip_nonfinite=False, logq=False, eval_neg=None, ctr_report=False, calibrate=False, tune_threshold=None):
    """train.py:16-109 on the GPU path.  ``data`` = the 16-tuple of mvin_amd.data_io.load_data / the
    reference's ``load_data`` (read by position exactly as train.py:17-21 does; a 10-tuple prefix
    (..., user_triplet_set) is accepted for CTR runs).  Per epoch: shuffle, full minibatches only
    (:56-64), then CTR evaluation on train/eval/test with early stopping on the eval AUC (:87-103) or,
    with ``show_topk``, top-K evaluation over the candidate set ``item_set_most_pop`` = data[12]
    (:69-77 pass it where topk_eval's signature says item_set) scored on eval recall@k_list[2].
    In top-K mode the reference NEVER stops early: :86 compares update_score's return value
    ('EarlyStopping' or None) with True.  That is reproduced (the best-epoch save still happens);
    ``topk_early_stop=True`` applies the evident intent instead (listed in INTEGRATION.md section 4).
    ``hoist``: evaluate through the entity-table mode (weights are frozen while an epoch is evaluated; the
    tables are dropped by every optimizer step and rebuilt by the first evaluation batch) -- 2-4x faster
    evaluation at the same tolerance; training steps always take the faithful kernels.
    ``graph``: replay every optimisation step as one hipGraph (training.GraphedTrainer; same kernels, losses read back
    once per epoch); "auto" = at batch sizes up to 2 048, where a step is launch- and latency-bound (the reference's
    scripts train at 512 / 1 024).
    ``topk_impl``: "host" ranks user by user on the host (topk_eval_device); "batched" ranks every user on the device in one
    call (topk_eval_batched; ties by ascending item id); "ranked" computes the same numbers as "batched", to the last bit, from
    the exact ranks of the truth items (topk_eval_ranked, mvin_rank_positives: no selection, no bound on k); "sampled" ranks
    every held-out interaction of the split against ``eval_neg`` (1..4095, default 99) sampled items instead of the candidate
    set (topk_eval_sampled, mvin_rank_segments; the same draw every epoch, seed ``args.neg_seed`` or 1): a fraction of the
    work, and SAMPLED numbers that are not comparable with the other three's.  ``eval_neg`` with any other ``topk_impl`` is
    refused.
    ``ctr_impl``: "host" evaluates CTR batch by batch with sklearn on the host (ctr_eval_device); "batched" scores each split
    into one device buffer and counts every batch's metrics exactly in one launch (ctr_eval_batched).
    ``negatives``: "fixed" trains on the label-0 rows ``train_data`` came with, every epoch; "resample" keeps the positives
    of ``train_data`` and draws one fresh negative per positive for every epoch on the device (data_prep.NegativeSampler with
    ``round`` = the epoch, seed ``args.neg_seed`` or 1; train_epoch_resampled), never an item the user has with label 1 in
    train, eval or test.  The per-epoch CTR evaluation of the train split still evaluates the fixed ``train_data``, which keeps
    the history comparable.  The draws depend on (seed, epoch) only: every rank of a multi-rank run builds the same epoch.
    ``objective``: "bce" trains on independent (user, item, label) rows with sigmoid cross-entropy, the reference's loss;
    "bpr" / "softmax" train every positive against ``n_neg`` (1..63) fresh negatives of the same user per epoch
    (train_epoch_ranked: groups of 1 + n_neg rows, ``args.batch_size // (1 + n_neg)`` groups per step) and need
    ``negatives="resample"``.  An opt-in extension (the reference trains with cross-entropy only); the epoch record gains
    "pairwise_acc", the sampled pairwise accuracy of the epoch's training steps.  Evaluation, early stopping and
    ``topk_impl`` are the same under every objective.
    ``negatives="hard"`` (with a ranking objective; single rank): dynamic negative sampling.  Every epoch draws ``pool`` (n_neg
    .. 63) fresh candidates per positive, scores them with the current weights and trains on ``n_neg`` of the ``shortlist``
    (n_neg .. pool; None = n_neg, the hardest; pool = uniform) highest-scored ones, picked on the device by
    mvin_select_negatives (train_epoch_hard); ``rescore`` = k scores and picks again before each k-th of the epoch.  The epoch
    record also gains "hard_rate" and "pool_rate": the share of the trained negatives, and of all pool candidates, that the
    model scored above their positive.
    ``neg_dist``: the distribution the sampler of ``negatives="resample"`` / ``"hard"`` draws from: "uniform" over the items the
    user has not watched, or "popularity": in proportion to (count_i + ``neg_smooth``) ** ``neg_alpha``, count_i = the label-1
    rows of ``train_data`` with item i (data_prep.NegativeSampler(dist=...), mvin_sample_negatives_weighted; an item of weight
    zero is never a negative).  It reaches every training mode through the sampler: cross-entropy epochs, the ranking
    objectives' groups and the hard-negative pool.  An opt-in extension, like the ranking objectives.
    ``logq``: True trains ``objective="softmax"`` with the logQ correction of a sampled softmax (Bengio & Senecal; Yi et al.
    2019): the log of every negative's expected sampling count under the sampler's proposal is subtracted from its logit
    before the softmax (train_epoch_ranked(logq=True), data_prep.rank_offsets, mvin_rank_head_offset), so that a
    popularity-weighted proposal (``neg_dist="popularity"``) no longer pushes popular items down by about log q, and the loss
    estimates the softmax over all of a user's eligible items under either proposal.  It needs ``negatives="resample"``;
    "bce" / "bpr" have no softmax to correct, fixed negatives have no known proposal, and ``negatives="hard"`` picks from a
    shortlist, a proposal this correction does not describe: each is refused.  The epoch record gains "logq": True;
    "pairwise_acc" still compares raw scores.  Opt-in; off, nothing changes.
    ``clip_norm`` / ``skip_nonfinite``: the guard of the optimizer step (training.Trainer.set_guard), set on the model's trainer
    before the first epoch: gradients clipped to the global norm ``clip_norm`` (a finite number > 0) and / or a step with a
    non-finite gradient left out, both decided on the device, so a step stays one graph replay.  With either set the epoch
    record gains "grad_norm": {"mean", "max"} (over the epoch's steps with a finite norm), "clipped_steps" and
    "skipped_steps", from one read-back per epoch; "loss" stays the mean over every step, so an epoch with skipped steps may
    show nan there -- "skipped_steps" says why.  An opt-in extension: off, the steps are exactly the unguarded ones.
    ``ctr_report``: True (with ``ctr_impl="batched"``, not with ``show_topk``) adds to every split's record the numbers of
    harness.ctr_report over the whole split: "logloss", "brier", "ece" and "gauc" ({"weighted", "mean", "users",
    "skipped_users"}); "auc" / "acc" / "f1" stay the per-batch means.  ``calibrate``: True (needs ``ctr_report``) fits a Platt
    map on the eval split every epoch (fit_calibration) and gives the test record "calibrated": {"a", "b", "logloss", "acc",
    "f1"} under that map.  An opt-in extension (the reference reports none of these): off, the records are exactly the ones
    without it.
    ``tune_threshold``: "f1", "acc" or "youden" (needs ``ctr_report``; None: off, the records are unchanged) picks the logit cut
    that maximises that criterion on the eval split every epoch (pick_threshold) and gives the test record "tuned":
    {"criterion", "threshold", "acc", "f1", "precision", "recall"}: the test split at that cut (ctr_report(threshold=)) -- the
    acc / F1 to read under the ranking objectives, whose logits are not centred on the fixed cut.
    ``on_best``: called as ``on_best(epoch, score, model)`` after every epoch whose evaluation score is above every earlier
    one's -- exactly where EarlyStop saves the stage-wise tables, whether or not ``args.path.emb`` is set.
    Returns (model, history): one dict per epoch."""
    if topk_impl not in ("host", "batched", "ranked", "sampled"):
        raise ValueError(f"topk_impl={topk_impl!r}: expected 'host', 'batched', 'ranked' or 'sampled'")
    if eval_neg is not None and topk_impl != "sampled":
        raise ValueError(f"eval_neg={eval_neg!r} is the number of sampled candidates of topk_impl='sampled', not of {topk_impl!r}")
    if topk_impl == "sampled":
        eval_neg = 99 if eval_neg is None else eval_neg
        if isinstance(eval_neg, (bool, np.bool_)) or int(eval_neg) != eval_neg or not 1 <= int(eval_neg) <= 4095:
            raise ValueError(f"eval_neg={eval_neg!r}: expected an integer in [1, 4095]")
    if ctr_impl not in ("host", "batched"):
        raise ValueError(f"ctr_impl={ctr_impl!r}: expected 'host' or 'batched'")
    if not isinstance(ctr_report, (bool, np.bool_)) or not isinstance(calibrate, (bool, np.bool_)):
        raise ValueError(f"ctr_report={ctr_report!r}, calibrate={calibrate!r}: expected True or False")
    if ctr_report and ctr_impl != "batched":
        raise ValueError(f"ctr_report=True reads the scores a split leaves on the device: it needs ctr_impl='batched', not {ctr_impl!r}")
    if ctr_report and show_topk:
        raise ValueError("ctr_report=True reports on the CTR evaluation, which show_topk=True replaces")
    if calibrate and not ctr_report:
        raise ValueError("calibrate=True reports the calibrated numbers in the CTR report: it needs ctr_report=True")
    if tune_threshold is not None:
        _check_criterion(tune_threshold, "train: tune_threshold")
        if show_topk:
            raise ValueError("tune_threshold tunes the cut of the CTR evaluation, which show_topk=True replaces")
        if not ctr_report:
            raise ValueError("tune_threshold reports the tuned numbers in the CTR report: it needs ctr_report=True")
    if negatives not in ("fixed", "resample", "hard"):
        raise ValueError(f"negatives={negatives!r}: expected 'fixed', 'resample' or 'hard'")
    if objective not in ("bce", "bpr", "softmax"):
        raise ValueError(f"objective={objective!r}: expected 'bce', 'bpr' or 'softmax'")
    if neg_dist not in ("uniform", "popularity"):
        raise ValueError(f"neg_dist={neg_dist!r}: expected 'uniform' or 'popularity'")
    if neg_dist != "uniform" and negatives == "fixed":
        raise ValueError(f"neg_dist={neg_dist!r} is the distribution of the per-epoch sampler: it needs negatives='resample' or 'hard'")
    from .training import check_clip_norm
    clip_norm = check_clip_norm(clip_norm)
    if not isinstance(skip_nonfinite, (bool, np.bool_)):
        raise ValueError(f"skip_nonfinite={skip_nonfinite!r}: expected True or False")
    guard = clip_norm is not None or bool(skip_nonfinite)
    if not isinstance(logq, (bool, np.bool_)):
        raise ValueError(f"logq={logq!r}: expected True or False")
    if logq:
        if objective != "softmax":
            raise ValueError(f"logq=True corrects the sampled softmax for its proposal: it needs objective='softmax', not "
                             f"{objective!r}" + (" (the kernel's BPR offset is a margin; the harness exposes none)"
                                                 if objective == "bpr" else ""))
        if negatives == "fixed":
            raise ValueError("logq=True needs the proposal the negatives were drawn from: negatives='fixed' rows have none, "
                             "use negatives='resample'")
        if negatives == "hard":
            raise ValueError("logq=True does not describe negatives='hard': picking from a scored shortlist changes the "
                             "proposal in a way the correction does not cover; use negatives='resample'")
    ranked = objective != "bce"
    hard = negatives == "hard"
    if hard and not ranked:
        raise ValueError("negatives='hard' picks the negatives of a ranking objective: it needs objective='bpr' or 'softmax'")
    if ranked:
        if negatives == "fixed":
            raise ValueError(f"objective={objective!r} draws its negatives per epoch: it needs negatives='resample' (or 'hard')")
        if int(n_neg) != n_neg or not 1 <= int(n_neg) <= 63:
            raise ValueError(f"n_neg={n_neg!r}: expected an integer in [1, 63]")
        if args.batch_size < 1 + int(n_neg):
            raise ValueError(f"batch_size={args.batch_size} holds no group of 1 + n_neg = {1 + int(n_neg)} rows")
    if hard:
        if int(pool) != pool or not int(n_neg) <= int(pool) <= 63:
            raise ValueError(f"pool={pool!r}: expected an integer in [n_neg = {int(n_neg)}, 63]")
        if shortlist is not None and (int(shortlist) != shortlist or not int(n_neg) <= int(shortlist) <= int(pool)):
            raise ValueError(f"shortlist={shortlist!r}: expected an integer in [n_neg = {int(n_neg)}, pool = {int(pool)}] or None")
        if int(rescore) != rescore or int(rescore) < 1:
            raise ValueError(f"rescore={rescore!r}: expected an integer >= 1")
    from .model import MVIN
    n_user, n_item, n_entity, n_relation = data[0], data[1], data[2], data[3]
    train_data, eval_data, test_data = (np.asarray(d) for d in data[4:7])
    adj_entity, adj_relation, uts = data[7], data[8], data[9]
    if model is None:
        model = MVIN(args, n_user, n_entity, n_relation, adj_entity, adj_relation, device=device, hoist=bool(hoist))
        if getattr(args, "load_pretrain_emb", False):
            model.restore_pretrain_emb()                                       # train.py:53-54
    feeder = DeviceFeeder(model, uts)
    stop = EarlyStop(getattr(args, "tolerance", 2), getattr(args, "early_stop", 3),
                     getattr(args, "save_final_model", True))
    stop.on_best = on_best
    if show_topk:
        user_list, train_rec, eval_rec, test_rec, item_set, k_list = topk_settings(train_data, eval_data, test_data,
                                                                                   n_item)
        if len(data) > 12 and data[12] is not None:
            item_set = set(int(i) for i in data[12])                            # item_set_most_pop, train.py:70,75
    history = []
    train_data = train_data.copy()
    sampler = None
    if negatives != "fixed":
        from .data_prep import NegativeSampler
        ratio = float(int(pool)) if hard else float(int(n_neg)) if ranked else 1.0
        dist_kw = {} if neg_dist == "uniform" else {"dist": neg_dist, "alpha": float(neg_alpha), "smooth": float(neg_smooth)}
        sampler = NegativeSampler(train_data, n_user, n_item, exclude=(eval_data, test_data), ratio=ratio,
                                  seed=getattr(args, "neg_seed", 1), device=model.device, **dist_kw)
    if not ranked and model.trainer is not None:
        model.trainer.set_objective("bce")
    if guard and model.trainer is None:
        from .training import Trainer
        model.trainer = Trainer(model)
    if model.trainer is not None:
        model.trainer.set_guard(clip_norm, bool(skip_nonfinite))
        if guard:
            model.trainer.guard_stats(reset=True)            # the epoch records count from here
    for epoch in range(getattr(args, "n_epochs", 20)):
        use_graph = (args.batch_size <= 2048) if graph == "auto" else bool(graph)
        if hard:
            losses = train_epoch_hard(feeder, sampler, args.batch_size, epoch, objective, int(n_neg), shortlist=shortlist,
                                      rescore=int(rescore), graph=use_graph)
        elif ranked:
            losses = train_epoch_ranked(feeder, sampler, args.batch_size, epoch, objective, graph=use_graph, logq=bool(logq))
        elif sampler is not None:
            losses = train_epoch_resampled(feeder, sampler, args.batch_size, epoch, graph=use_graph)
        else:
            losses = train_epoch_device(feeder, train_data, args.batch_size, rng=rng, graph=use_graph)
        rec = {"epoch": epoch, "loss": float(np.mean(losses)) if losses else float("nan")}
        if ranked:
            rec["pairwise_acc"] = model.trainer.last_pairwise_acc
        if logq:
            rec["logq"] = True
        if hard:
            rec["hard_rate"], rec["pool_rate"] = model.trainer.last_hard_rate, model.trainer.last_pool_rate
        if guard:
            gs = model.trainer.guard_stats(reset=True)
            rec["grad_norm"] = {"mean": gs["norm_mean"], "max": gs["norm_max"]}
            rec["clipped_steps"], rec["skipped_steps"] = gs["clipped_steps"], gs["skipped_steps"]
        if show_topk:
            for mode in ("eval", "test"):
                if topk_impl == "sampled":
                    p, r, n, _, _ = topk_eval_sampled(feeder, train_data, eval_data, test_data, n_user, n_item, k_list, mode=mode,
                                                      n_neg=int(eval_neg), seed=getattr(args, "neg_seed", 1))
                elif topk_impl in ("batched", "ranked"):
                    topk = topk_eval_ranked if topk_impl == "ranked" else topk_eval_batched
                    p, r, n, _, _ = topk(feeder, user_list, train_rec, eval_rec, test_rec, item_set, k_list, mode=mode)
                else:
                    p, r, n, _, _ = topk_eval_device(feeder, user_list, train_rec, eval_rec, test_rec, item_set, k_list,
                                                     topk_batch, mode=mode)
                rec[mode] = {"precision": p, "recall": r, "ndcg": n}
            score = rec["eval"]["recall"][2]
        else:
            for name, d in (("train", train_data), ("eval", eval_data), ("test", test_data)):
                ctr = ctr_eval_batched if ctr_impl == "batched" else ctr_eval_device
                _, _, _, auc, acc, f1 = ctr(feeder, d, args.batch_size)
                rec[name] = {"auc": auc, "acc": acc, "f1": f1}
                if ctr_report:
                    rep = _ctr_report(feeder, d)
                    rec[name].update({k: rep[k] for k in ("logloss", "brier", "ece", "gauc")})
            if calibrate:
                cal = fit_calibration(feeder, eval_data, name="the eval split")
                rep = _ctr_report(feeder, test_data, calibration=cal, gauc=False)
                rec["test"]["calibrated"] = {"a": cal.a, "b": cal.b, "logloss": rep["logloss"], "acc": rep["acc"], "f1": rep["f1"]}
            if tune_threshold is not None:
                at = _ctr_report(feeder, test_data, threshold=pick_threshold(feeder, eval_data, tune_threshold), gauc=False)["at_threshold"]
                rec["test"]["tuned"] = dict({"criterion": tune_threshold}, **{k: at[k] for k in ("threshold", "acc", "f1", "precision", "recall")})
            score = rec["eval"]["auc"]                                          # Eval_score_info.eval_st_score
        history.append(rec)
        if log:
            log(rec)
        if stop.update(epoch, score, model) and (topk_early_stop or not show_topk):
            break
    return model, history


# --------------------------------------------------------------------------- stage-wise training (main.py:24-45)
def stage_seeds(sampling_seed, stage):
    """(adjacency seed, ripple-set seed) of stage ``stage``: sampling_seed + 1 + 2 * stage and sampling_seed + 2 + 2 * stage.
    At stage 0 these are the seeds data_io.load_data(seed=sampling_seed) draws with."""
    return int(sampling_seed) + 1 + 2 * int(stage), int(sampling_seed) + 2 + 2 * int(stage)


class StageTracker(object):
    """The book-keeping of the reference's stage-wise loop (main.py:24-45 with train_util.py's Train_info_record_sw_emb /
    Train_info_record_emb_sw_ndcg), without its log files.  Pure Python.

    Within a stage the epoch with the highest evaluation score counts -- eval AUC, or with ``show_topk`` eval recall at
    k_list[2]; strict ``>``, starting from 0 (update_score) -- and its test metrics are the stage's.  Across stages
    (train_over) a stage whose score is strictly above the best so far becomes the best and resets the miss counter; any other
    stage, one that only EQUALS the best included, counts as a miss.  ``end_stage`` says stop once ``patience`` misses have
    accumulated -- looked at after a restart only, as main.py:42 does, so stage 1 always runs -- or after ``max_stages``
    restarts.  Feed it ``start_stage()``, ``epoch(rec)`` with every record of harness.train's history, ``end_stage()``."""

    def __init__(self, max_stages=5, patience=3, show_topk=False):
        self.max_stages, self.patience, self.show_topk = int(max_stages), int(patience), bool(show_topk)
        self.stage = -1
        self.misses = 0
        self.best_stage, self.best_score, self.best_eval, self.best_test = None, 0, None, None
        self.records = []
        self._cur = None

    def score_of(self, rec):
        return rec["eval"]["recall"][2] if self.show_topk else rec["eval"]["auc"]

    def start_stage(self):
        self.stage += 1
        self._cur = {"stage": self.stage, "score": 0, "best_epoch": None, "eval": None, "test": None}
        return self.stage

    def epoch(self, rec):
        """True when ``rec`` is the stage's best epoch so far."""
        score = self.score_of(rec)
        if score > self._cur["score"]:
            self._cur.update(score=score, best_epoch=rec.get("epoch"), eval=rec["eval"], test=rec["test"])
            return True
        return False

    def end_stage(self):
        """Close the stage; True when the loop stops here."""
        cur = self._cur
        if cur["score"] > self.best_score:
            self.best_stage, self.best_score, self.best_eval, self.best_test = cur["stage"], cur["score"], cur["eval"], cur["test"]
            self.misses = 0
        else:
            self.misses += 1
        cur["misses"] = self.misses
        self.records.append(cur)
        return (self.stage >= 1 and self.misses >= self.patience) or self.stage >= self.max_stages


class StagewiseResult(object):
    """What train_stagewise returns beside the model and the feeder: ``stages`` (one dict per stage run), ``best_stage`` (the
    index of the stage whose best epoch the model holds), ``best_eval`` / ``best_test`` (that epoch's metrics: the numbers the
    reference publishes) and ``use_neighbor_rate`` ([field_edges, explored_total, rate] or None)."""

    def __init__(self, stages, tracker, use_neighbor_rate):
        self.stages, self.tracker = stages, tracker
        self.best_stage, self.best_eval, self.best_test = tracker.best_stage, tracker.best_eval, tracker.best_test
        self.use_neighbor_rate = use_neighbor_rate


def train_stagewise(args, data, kg, *, max_stages=5, patience=3, show_topk=False, sampling_seed=1, init_seed=0,
                    resample_first=False, explore=True, on_stage=None, device="cuda", log=None, **train_kw):
    """Stage-wise training, the procedure of main.py:24-45: train stage 0, then restart up to ``max_stages`` times.  Every
    restart draws a fresh sampled adjacency and fresh ripple sets on the device, builds a new model, copies the four ``_STWS``
    embedding tables in from the best epoch of the stage before, and trains again; the loop stops after ``patience`` stages
    without a better evaluation score (StageTracker).  The published number is the test score of the best stage's best epoch.

    ``data``: harness.train's tuple; ``kg``: the [n, 3] (h, r, t) triples or a data_prep.build_csr triple.  For stage s:
      * inputs: stage 0 trains on data[7:10] as given unless ``resample_first``; every other stage draws
        construct_adj(seed = sampling_seed + 1 + 2 s) and get_user_triplet_set(seed = sampling_seed + 2 + 2 s) (``stage_seeds``;
        at s = 0 that is what data_io.load_data(seed=sampling_seed) draws).  The train / eval / test split stays FIXED: the
        reference re-splits with an unseeded generator on every restart, which leaks test rows into training;
      * model: a fresh MVIN(seed = init_seed + s) -- every other parameter and the Adam state start over, as the reference's
        new graph and global initialiser do -- with, for s > 0, the STWS tables of the PREVIOUS stage's best epoch (not the
        best stage's: the reference's checkpoint file is overwritten by the first epoch of every stage).  args.SW_stage = s;
      * training: one harness.train(args, stage_data, model=model, show_topk=..., **train_kw) call; its ``on_best`` hook keeps
        device clones of all parameters at the stage's best epoch.  The file checkpoint works as before when args.path.emb is set;
      * exploration (``explore``): a data_prep.KGExploration over the items of the train split and hops = tree_depth(args),
        updated with every stage's adjacency; the stage record carries field_edges, explored_now, new_edges, explored_total,
        rate, and args.use_neighbor_rate = [field_edges, explored_total, round(rate, 6)].
    ``on_stage(stage, model, feeder, record)`` is called before a stage trains; ``log`` receives every epoch record
    (harness.train) and, after each stage, the stage record without its history.  Returns (model, feeder, result): the model as
    it was at the best epoch of the best stage, with that stage's adjacency re-installed (redrawn from its seed) and a
    DeviceFeeder over that stage's ripple sets; ``result``: a StagewiseResult."""
    import torch
    from . import data_prep
    from .config import tree_depth
    from .model import MVIN
    n_user, n_item, n_entity, n_relation = data[0], data[1], data[2], data[3]
    train_data = np.asarray(data[4])
    K, P, Nm = args.neighbor_sample_size, args.p_hop, args.n_memory
    if isinstance(kg, (tuple, list)) and len(kg) == 3 and all(torch.is_tensor(t) for t in kg):
        csr = tuple(kg)
    else:
        csr = data_prep.build_csr(kg, n_entity, device=device)
    hist = data_prep.history_csr(train_data, n_user, device=device)
    hoist = bool(train_kw.pop("hoist", True))

    def draw(stage):
        seed_adj, seed_uts = stage_seeds(sampling_seed, stage)
        return (data_prep.construct_adj(csr, n_entity, K, seed=seed_adj),
                data_prep.get_user_triplet_set(csr, hist, n_user, P, Nm, seed=seed_uts))

    expl = data_prep.KGExploration(csr, train_data[:, 1], tree_depth(args)) if explore else None
    tracker = StageTracker(max_stages, patience, show_topk)
    stages, snaps, prev = [], {}, None
    while True:
        s = tracker.start_stage()
        given = s == 0 and not resample_first
        if given:
            adj_e, adj_r, uts = data[7], data[8], data[9]
        else:
            (adj_e, adj_r), uts = draw(s)
        args.SW_stage = s
        model = MVIN(args, n_user, n_entity, n_relation, adj_e, adj_r, device=device, seed=init_seed + s, hoist=hoist)
        if prev is not None:
            model.load_stws(prev)
        record = {"stage": s, "seed_adj": None if given else stage_seeds(sampling_seed, s)[0],
                  "seed_uts": None if given else stage_seeds(sampling_seed, s)[1], "init_seed": init_seed + s}
        if expl is not None:
            now, new, total = expl.update(model.adj_entity, model.adj_relation)
            record.update(field_edges=expl.field_edges, explored_now=now, new_edges=new, explored_total=total, rate=expl.rate)
            args.use_neighbor_rate = [expl.field_edges, total, round(expl.rate, 6)]
        feeder = DeviceFeeder(model, uts)
        if on_stage is not None:
            on_stage(s, model, feeder, record)
        best = {}

        def keep(epoch, score, m, best=best):
            best.update(epoch=epoch, score=score, state=m.state())

        stage_data = tuple(data[:7]) + (model.adj_entity, model.adj_relation, feeder.uts) + tuple(data[10:])
        _, history = train(args, stage_data, show_topk=show_topk, model=model, device=device, log=log, hoist=hoist,
                           on_best=keep, **train_kw)
        for rec in history:
            tracker.epoch(rec)
        stop = tracker.end_stage()
        cur = tracker.records[-1]
        record.update(history=history, best_epoch=cur["best_epoch"], score=cur["score"], eval=cur["eval"], test=cur["test"],
                      misses=cur["misses"])
        stages.append(record)
        prev = best.get("state")
        snaps[s] = (prev, (model.adj_entity, model.adj_relation, feeder.uts) if given else None)
        for old in list(snaps):                    # only the best stage's snapshot is needed again
            if old != s and old != tracker.best_stage:
                del snaps[old]
        if log:
            log({k: v for k, v in record.items() if k != "history"})
        if stop:
            break
    b = tracker.best_stage if tracker.best_stage is not None else s       # no stage ever scored above 0: the last one
    state, inputs = snaps[b]
    if b != s:                                     # the last model object carries on, as the best stage's model
        if inputs is None:
            (adj_e, adj_r), uts = draw(b)
        else:
            adj_e, adj_r, uts = inputs
        model.set_adjacency(adj_e, adj_r)
        feeder = DeviceFeeder(model, uts)
    if state is not None:
        model.load_state(state)
    model.trainer = None                           # its moments belong to the last stage's run, not to these parameters
    model._graphed_trainer = None
    args.SW_stage = b
    return model, feeder, StagewiseResult(stages, tracker, getattr(args, "use_neighbor_rate", None) if explore else None)


# --------------------------------------------------------------------------- case study (f-4)
def _names(ids, table):
    return [table[str(i)] if str(i) in table else str(i) for i in ids]


def ctr_eval_case_study(args, model, data, user_triplet_set, user_history_dict, entity_index_2_name,
                        rela_index_2_name, user_list, item_set_most_pop, batch_size, path, sess=None):
    """util.py:59-127: dump sampled neighbors, relations and attention weights per selected
    (user, item) pair in the reference's text layout.  Written to ``path`` (the reference derives
    the file name from args.path.case_st / log_name / epoch / SW_stage)."""
    nb = args.neighbor_sample_size
    star20, star50 = "*" * 20, "*" * 50
    with open(path, "w") as f:
        f.write(f"{star50}\n case_study \n")
        start = 0
        while start + batch_size <= data.shape[0]:
            users, labels, items, ents, rels, imp0, imp1 = model.eval_case_study(
                sess, get_feed_dict(args, model, data, user_triplet_set, start, start + batch_size))
            for b in range(batch_size):
                if users[b] not in user_list or items[b] not in item_set_most_pop:
                    continue
                f.write(f"{star50}\n")
                f.write(f"user_indices = {users[b]}, item_indices = {items[b]}, labels = {labels[b]}\n")
                f.write(f"{star20} first_layer  {star20}\n")
                f.write(f"et_index 0 = {','.join(str(x) for x in ents[0][b, :].tolist())}\n")
                f.write(f"rela_index 0 = {','.join(str(x) for x in rels[0][b, :].tolist())}\n")
                f.write(f"et_index 1 = {','.join(str(x) for x in ents[1][b, :].tolist())}\n")
                f.write(f"{star20} second_layer  {star20}\n")
                for k in range(nb):
                    f.write(f"entities 0 = {k}\n")
                    f.write(f"et_index 0 = {ents[1][b, k].tolist()}\n")
                    f.write(f"rela_index 0 = {','.join(str(x) for x in rels[1][b, nb * k: nb * (k + 1)].tolist())}\n")
                    f.write(f"et_index 1 = {','.join(str(x) for x in ents[2][b, nb * k: nb * (k + 1)].tolist())}\n")
                f.write(f"{star20} entity_relation_name  {star20}\n")
                hist = _names(user_history_dict.get(users[b], []), entity_index_2_name)
                f.write(f"item_name = {_names([items[b]], entity_index_2_name)[0]}\n")
                f.write(f"user_interact_items = {','.join(hist)}\n")
                ename = [_names(e[b, :], entity_index_2_name) for e in ents]
                rname = [_names(r[b, :], rela_index_2_name) for r in rels]
                f.write(f"{star20} first_layer  {star20}\n")
                f.write(f"et_index 0 = {','.join(ename[0])}\n")
                pairs = ["rela = %s, enti = %s, att = %s" % p for p in zip(rname[0], ename[1], imp0[b, :][0])]
                f.write("er rela pair 0 = " + "\n".join(pairs) + "\n")
                f.write(f"{star20} second_layer  {star20}\n")
                for k in range(nb):
                    f.write(f"entities 0 = {k}\n")
                    f.write(f"et_index 0 = {ename[1][k]}\n")
                    pairs = ["rela = %s, enti = %s, att = %s" % p for p in
                             zip(rname[1][nb * k: nb * (k + 1)], ename[2][nb * k: nb * (k + 1)], imp1[b, k])]
                    f.write("er rela pair 1 = " + "\n".join(pairs) + "\n")
            start += batch_size


# --------------------------------------------------------------------------- explaining a score (an extension beside f-4)
def explain_pairs(feeder, users, items, top, entity_names=None, relation_names=None):
    """``DeviceFeeder.explain`` as plain Python records for printing: one dict per pair with ``user``, ``item``, ``item_name``,
    ``score``, ``distinct`` (its number of distinct paths), ``total_weight`` (the sum of all its path weights; 1 up to the
    float32 rounding of the two softmaxes) and ``paths``, the up to ``top`` heaviest distinct paths, heaviest first: dicts with
    ``relations`` / ``entities`` (ids: (rel0, rel1) / (ent1, ent2); one entry each at depth 1), ``relation_names`` /
    ``entity_names`` (through the lookup ``ctr_eval_case_study`` uses: ``table[str(id)]``, the id itself where the table has
    none), ``weight`` (mass / 2^40), ``share`` (mass / the pair's total mass), ``mass`` and ``slot``.  Everything comes back in
    ONE copy."""
    import torch
    res = feeder.explain(users, items, top=top)
    B, top = res["mass"].shape
    two = feeder.model.n_mix_hop * feeder.model.h_hop >= 2
    packed = torch.cat([res["paths"].reshape(B, top * 4).long(), res["mass"], res["slot"].long(), res["distinct"].long()[:, None],
                        res["total"][:, None], res["scores"].view(torch.int32).long()[:, None],
                        _dev_ids(users, res["mass"].device)[:, None], _dev_ids(items, res["mass"].device)[:, None]], dim=1).cpu().numpy()
    ent_tab = entity_names if entity_names is not None else {}
    rel_tab = relation_names if relation_names is not None else {}
    scale = float(1 << 40)
    records = []
    for row in packed:
        paths, mass, slot = row[:top * 4].reshape(top, 4), row[top * 4:top * 5], row[top * 5:top * 6]
        distinct, total, score_bits, user, item = (int(x) for x in row[top * 6:top * 6 + 5])
        listed = []
        for p in range(min(top, distinct)):
            rel_ids = [int(paths[p, 0])] + ([int(paths[p, 2])] if two else [])
            ent_ids = [int(paths[p, 1])] + ([int(paths[p, 3])] if two else [])
            listed.append(dict(relations=rel_ids, entities=ent_ids, relation_names=_names(rel_ids, rel_tab),
                               entity_names=_names(ent_ids, ent_tab), weight=int(mass[p]) / scale,
                               share=int(mass[p]) / total if total else 0.0, mass=int(mass[p]), slot=int(slot[p])))
        records.append(dict(user=user, item=item, item_name=_names([item], ent_tab)[0],
                            score=float(np.int32(score_bits).view(np.float32)), distinct=distinct, total_weight=total / scale,
                            paths=listed))
    return records


def relation_profile(feeder, data, batch_size):
    """The share of attention mass per relation over a split: ``data`` [n, >= 2] rows of (user, item, ...), explained in
    batches of ``batch_size`` pairs (``DeviceFeeder.explain(..., profile=True)``), the integer masses of both levels summed
    over the batches.  Returns ``dict(mass int64 [2, n_relation], share float64 [2, n_relation], n_pairs)`` on the host: row 0
    the level-1 slots (item -> neighbour), row 1 the path slots (neighbour -> neighbour's neighbour; all zero at depth 1);
    ``share`` = a row of ``mass`` over its sum (zeros where the sum is 0)."""
    data = np.asarray(data)
    res = feeder.explain(data[:, 0], data[:, 1], top=1, profile=True, max_pairs=int(batch_size))
    mass = res["rel_mass"].cpu().numpy()
    tot = mass.sum(axis=1, keepdims=True)
    share = np.divide(mass.astype(np.float64), tot, out=np.zeros(mass.shape, np.float64), where=tot > 0)
    return dict(mass=mass, share=share, n_pairs=int(data.shape[0]))


def explain_user_memories(feeder, users, items, top, entity_names=None, relation_names=None):
    """``DeviceFeeder.explain_memories`` as plain Python records for printing, shaped like ``explain_pairs``: one dict per pair
    with ``user``, ``item``, ``item_name``, ``score`` (the raw logit), ``score_normalized`` (its sigmoid), ``bias`` (the bias
    term of the logit) and ``blocks``, one dict per read of the user's ripple sets: ``block`` ("h_set", "hop0", ...),
    ``contribution`` (the block's share of the logit), ``distinct``, ``total_weight`` and ``memories``, the up to ``top``
    heaviest distinct memories, heaviest first: dicts with ``block``, ``h`` / ``r`` / ``t`` (ids; r and t None in the h-set
    block), ``h_name`` / ``r_name`` / ``t_name`` (through the lookup ``explain_pairs`` uses), ``weight`` (mass / 2^40),
    ``contribution`` (signed, in logit units), ``share`` (contribution / score; 0 where the score is 0), ``mass`` and ``slot``.
    Everything comes back in ONE copy."""
    import torch
    res = feeder.explain_memories(users, items, top=top)
    B, n_o, top = res["mass"].shape
    dev = res["mass"].device
    bits = lambda t: t.reshape(B, -1).contiguous().view(torch.int32).long()              # f32 -> its bits, exactly
    packed = torch.cat([res["mem"].reshape(B, n_o * top * 3).long(), res["mass"].reshape(B, -1), res["slot"].reshape(B, -1).long(),
                        bits(res["contrib"]), res["distinct"].long(), res["total"], bits(res["score_parts"]), bits(res["scores"]),
                        bits(res["scores_normalized"]), _dev_ids(users, dev)[:, None], _dev_ids(items, dev)[:, None]],
                       dim=1).cpu().numpy()
    f32 = lambda x: np.asarray(x, np.int64).astype(np.int32).view(np.float32)
    ent_tab = entity_names if entity_names is not None else {}
    rel_tab = relation_names if relation_names is not None else {}
    has_set = bool(feeder.model.args.PS_O_ft)
    names = (["h_set"] if has_set else []) + [f"hop{i}" for i in range(n_o - (1 if has_set else 0))]
    scale = float(1 << 40)
    n = n_o * top
    records = []
    for row in packed:
        mem, mass, slot, contrib, distinct, total, parts, tail = np.split(row, np.cumsum([3 * n, n, n, n, n_o, n_o, n_o + 1]))
        mem, mass, slot, contrib = mem.reshape(n_o, top, 3), mass.reshape(n_o, top), slot.reshape(n_o, top), f32(contrib).reshape(n_o, top)
        parts = f32(parts)
        score, sig = (float(x) for x in f32(tail[:2]))
        user, item = int(tail[2]), int(tail[3])
        blocks = []
        for c in range(n_o):
            listed = []
            for p in range(min(top, int(distinct[c]))):
                h, r, t = (int(x) for x in mem[c, p])
                hop = names[c] != "h_set"
                listed.append(dict(block=names[c], h=h, r=r if hop else None, t=t if hop else None,
                                   h_name=_names([h], ent_tab)[0], r_name=_names([r], rel_tab)[0] if hop else None,
                                   t_name=_names([t], ent_tab)[0] if hop else None, weight=int(mass[c, p]) / scale,
                                   contribution=float(contrib[c, p]), share=float(contrib[c, p]) / score if score else 0.0,
                                   mass=int(mass[c, p]), slot=int(slot[c, p])))
            blocks.append(dict(block=names[c], contribution=float(parts[c]), distinct=int(distinct[c]),
                               total_weight=int(total[c]) / scale, memories=listed))
        records.append(dict(user=user, item=item, item_name=_names([item], ent_tab)[0], score=score, score_normalized=sig,
                            bias=float(parts[n_o]), blocks=blocks))
    return records


def memory_relation_profile(feeder, data, batch_size):
    """The share of ripple-set attention mass per relation and hop over a split, mirroring ``relation_profile``: ``data``
    [n, >= 2] rows of (user, item, ...), explained in batches of ``batch_size`` pairs
    (``DeviceFeeder.explain_memories(..., profile=True)``), the integer masses summed over the batches.  Returns ``dict(mass
    int64 [P, n_relation], share float64 [P, n_relation], n_pairs)`` on the host: row i the memories of hop i; ``share`` = a
    row of ``mass`` over its sum (zeros where the sum is 0).  The h-set read has no relation and is not part of it."""
    data = np.asarray(data)
    res = feeder.explain_memories(data[:, 0], data[:, 1], top=1, profile=True, max_pairs=int(batch_size))
    mass = res["rel_mass"].cpu().numpy()
    tot = mass.sum(axis=1, keepdims=True)
    share = np.divide(mass.astype(np.float64), tot, out=np.zeros(mass.shape, np.float64), where=tot > 0)
    return dict(mass=mass, share=share, n_pairs=int(data.shape[0]))


# the matrix-factorisation baseline and retrieval tower (mf.py, which builds on DeviceFeeder above): re-exported on first use
_MF_NAMES = ("MFModel", "MFTrainer", "MFFeeder", "train_mf")


def __getattr__(name):
    if name in _MF_NAMES:
        from . import mf
        return getattr(mf, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
