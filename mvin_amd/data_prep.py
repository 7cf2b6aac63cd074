"""Inputs of the scoring path built on the GPU (scope row f-1): counterparts of
construct_kg / contruct_random_adj / get_user_triplet_set
(src/model/MVIN/data_loader_user_set.py:324-343, :375-388, :392-441).

The reference builds these with pure-Python dict loops (minutes on amazon-book, repeated for
every stage-wise restart, main.py:16).  Here the KG becomes a CSR on the device (torch sort =
plumbing), and the two samplers are HIP kernels (mvin_sample_adjacency, mvin_build_ripple_sets)
whose draws are a pure function of a seed, so adjacency can be re-sampled every epoch.  The training negatives
(convert_rating, KGCN/preprocess.py:60-70) are drawn the same way by mvin_sample_negatives (sample_negatives,
NegativeSampler), fresh for every epoch -- uniformly, or in proportion to popularity^alpha from an alias table
(alias_table, mvin_sample_negatives_weighted).  KGExploration counts, exactly and on the device, how much of the KG within the
model's receptive field the sampled adjacencies have covered (mvin_kg_field / mvin_kg_explore): the number that says whether
another stage-wise restart, with its fresh adjacency, can show the model anything new.
"""
import numpy as np
import torch

from . import _lib
from .ops import _p, _stream


def build_csr(kg, n_entity, device="cuda"):
    """construct_kg (:324-343): treat the KG as undirected; every triple (h, r, t) is listed
    under h as (t, r) and under t as (h, r), in file order (head entry before tail entry).
    Returns (indptr int64 [nE+1], dst int32 [2n], rel int32 [2n]) on ``device``."""
    kg = torch.as_tensor(np.asarray(kg), dtype=torch.int64).to(device)
    n = kg.shape[0]
    src = torch.stack([kg[:, 0], kg[:, 2]], dim=1).reshape(-1)      # interleaved: h_0, t_0, h_1, t_1 ...
    dst = torch.stack([kg[:, 2], kg[:, 0]], dim=1).reshape(-1)
    rel = torch.stack([kg[:, 1], kg[:, 1]], dim=1).reshape(-1)
    order = torch.sort(src, stable=True).indices                    # keeps insertion order per entity
    deg = torch.bincount(src, minlength=n_entity)
    indptr = torch.zeros(n_entity + 1, dtype=torch.int64, device=kg.device)
    indptr[1:] = torch.cumsum(deg, 0)
    del n
    return indptr.contiguous(), dst[order].to(torch.int32).contiguous(), rel[order].to(torch.int32).contiguous()


def construct_adj(csr, n_entity, K, seed=1):
    """contruct_random_adj (:375-388) -> (adj_entity, adj_relation) int32 [nE, K] on the device."""
    indptr, dst, rel = csr
    lib = _lib.load()
    if dst.numel() == 0:      # a KG without triples: every entity keeps the all-zero row of :377-380 (found by the prep fuzz test)
        z = torch.zeros((n_entity, K), dtype=torch.int32, device=indptr.device)
        return z, z.clone()
    adj_e = torch.empty((n_entity, K), dtype=torch.int32, device=indptr.device)
    adj_r = torch.empty((n_entity, K), dtype=torch.int32, device=indptr.device)
    _lib.check(lib.mvin_sample_adjacency(_p(indptr), _p(dst), _p(rel), n_entity, K, seed, _p(adj_e), _p(adj_r),
                                         _stream()), "mvin_sample_adjacency")
    return adj_e, adj_r


def history_csr(train_data, n_user, device="cuda"):
    """user_history_dict of load_rating (data_loader_user_set.py:74-85) as CSR: each user's
    positive train items in interaction order."""
    d = np.asarray(train_data)
    pos = d[d[:, 2] == 1]
    order = np.argsort(pos[:, 0], kind="stable")
    users, items = pos[order, 0], pos[order, 1]
    ptr = np.zeros(n_user + 1, dtype=np.int64)
    np.add.at(ptr, users + 1, 1)
    np.cumsum(ptr, out=ptr)
    return (torch.from_numpy(ptr).to(device), torch.from_numpy(items.astype(np.int32)).to(device))


def get_user_triplet_set(csr, hist, n_user, p_hop, n_memory, seed=1, n_neighbor=16):
    """get_user_triplet_set (:392-441) -> int32 [n_user, max(1,P), 3, n_memory] on the device
    (the layout mvin_amd.harness.DeviceFeeder consumes).  Users without positive items keep
    zero rows (the reference simply has no entry for them)."""
    indptr, dst, rel = csr
    hist_ptr, hist_items = hist
    P = max(1, p_hop)
    lib = _lib.load()
    out = torch.zeros((n_user, P, 3, n_memory), dtype=torch.int32, device=indptr.device)
    if hist_items.numel() == 0 or dst.numel() == 0:     # nobody has a positive item / the KG has no triples: no entries
        return out
    _lib.check(lib.mvin_build_ripple_sets(_p(indptr), _p(dst), _p(rel), _p(hist_ptr), _p(hist_items), n_user, P,
                                          n_memory, n_neighbor, seed, _p(out), _stream()),
               "mvin_build_ripple_sets")
    return out


# --------------------------------------------------------------------------- training negatives
def _interaction_csr_host(rows, n_user, labels=1):
    """(ptr int64 [nU+1], ids int32) on the host: user u's row = the DISTINCT items u is listed with in any of ``rows``
    ([n, 3] (user, item, label) arrays) under label ``labels`` (None: under any label), ascending."""
    if isinstance(rows, np.ndarray) or torch.is_tensor(rows):
        rows = [rows]
    parts = []
    for r in rows:
        r = np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64).reshape(-1, 3)
        parts.append(r[:, :2] if labels is None else r[r[:, 2] == labels, :2])
    ui = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int64)
    if ui.shape[0] and (ui[:, 0].min() < 0 or ui[:, 0].max() >= n_user):
        raise ValueError(f"interaction_csr: user ids outside [0, {n_user})")
    if ui.shape[0] and (ui[:, 1].min() < -(1 << 31) or ui[:, 1].max() >= (1 << 31)):
        raise ValueError("interaction_csr: item ids do not fit int32")
    ui = np.unique(ui, axis=0)                                   # sorted by (user, item), duplicates dropped
    ptr = np.zeros(n_user + 1, dtype=np.int64)
    np.add.at(ptr, ui[:, 0] + 1, 1)
    np.cumsum(ptr, out=ptr)
    return ptr, np.ascontiguousarray(ui[:, 1].astype(np.int32))


def interaction_csr(rows, n_user, device="cuda", labels=1):
    """The per-user exclusion list of ``sample_negatives`` as a device CSR pair (ptr int64 [nU+1], ids int32) from any number
    of [n, 3] (user, item, label) arrays: every item a user has with label 1 in any of them -- or, with ``labels=None``, every
    item the user is listed with at all, which is convert_rating's ``item_set - pos - neg`` (KGCN/preprocess.py:60-70) for a
    caller with explicit negatives.  Rows come out ascending and distinct.  Host plumbing, like ``history_csr``."""
    ptr, ids = _interaction_csr_host(rows, n_user, labels)
    return torch.from_numpy(ptr).to(device), torch.from_numpy(ids).to(device)


def alias_table(weights, n_item=None):
    """The alias table of mvin_sample_negatives_weighted for non-negative ``weights`` [n_item] (Vose's construction in float64
    on the host, once per sampler; host plumbing like ``interaction_csr``).  Returns numpy arrays
    (tab uint32 [n_item, 2] = {thresh, alias} per bucket, mask uint32 [ceil(n_item / 32)]):
      * p_i = w_i * n_item / sum(w); the worklists of the items with p < 1 and with p >= 1 are processed in ascending item
        order (an item that drops below 1 joins the end of the first list), so the table is a pure function of ``weights``;
      * thresh = min(floor(p * 2^32), 2^32 - 1); a bucket that keeps probability 1 aliases to itself;
      * a zero-weight item gets its mask bit set (bit i % 32 of word i / 32) and thresh = 0, and no bucket aliases to it: it is
        never produced, and the mask makes it ineligible even if it were.
    What one draw really produces is ``alias_probabilities(tab)``.  ValueError for weights that are negative, non-finite, all
    zero, not one-dimensional, empty or (with ``n_item``) of another length."""
    w = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)
    if w.ndim != 1 or w.size == 0 or (n_item is not None and w.size != int(n_item)):
        raise ValueError(f"alias_table: weights of shape {w.shape}, expected ({'n_item' if n_item is None else int(n_item)},)")
    if not np.isfinite(w).all():
        raise ValueError("alias_table: weights must be finite")
    if (w < 0).any():
        raise ValueError("alias_table: weights must not be negative")
    total = float(w.sum())
    if not total > 0.0 or not np.isfinite(total):
        raise ValueError("alias_table: the weights are all zero (or their sum overflows)")
    n = w.size
    p = (w * (n / total)).tolist()
    alias = list(range(n))
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if p[i] >= 1.0]
    si = li = 0
    while si < len(small) and li < len(large):
        s, l = small[si], large[li]
        si += 1
        alias[s] = l
        p[l] = (p[l] + p[s]) - 1.0
        if p[l] < 1.0:
            small.append(l)
            li += 1
    for i in large[li:]:
        p[i] = 1.0
    heaviest = int(np.argmax(w))
    for i in small[si:]:                    # left over by round-off only: p is 1 up to that round-off
        if w[i] > 0.0:
            p[i] = 1.0
        else:                               # (a zero-weight item never keeps a share, whatever the round-off)
            alias[i] = heaviest
    thresh = np.minimum(np.floor(np.clip(np.asarray(p, dtype=np.float64), 0.0, 1.0) * 4294967296.0), 4294967295.0)
    thresh[w == 0.0] = 0.0
    tab = np.stack([thresh.astype(np.uint32), np.asarray(alias, dtype=np.uint32)], axis=1)
    bits = np.zeros(((n + 31) // 32) * 32, dtype=np.uint32)
    bits[:n] = w == 0.0
    mask = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(tab), np.ascontiguousarray(mask)


def alias_probabilities(tab, exact=False):
    """The probability with which ONE draw of mvin_sample_negatives_weighted produces each item, from the integers of
    ``tab`` (uint32 [n_item, 2]): bucket i is hit by mass(i) = ceil((i + 1) 2^32 / n_item) - ceil(i 2^32 / n_item) of the 2^32
    values of r0 (the multiply-high), keeps thresh[i] of the 2^32 values of r1 and sends the others to
    min(alias[i], n_item - 1).  Returns float64 [n_item] (the exact numerators over 2^64, rounded once); ``exact=True``
    returns the numerators as Python integers (they sum to 2^64).  This is what tests and documents compare against, not
    the float weights the table was built from."""
    t = np.asarray(tab.cpu() if torch.is_tensor(tab) else tab)
    if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] == 0:
        raise ValueError(f"alias_probabilities: tab of shape {t.shape}, expected (n_item, 2)")
    n = t.shape[0]
    edges = [-((-(i << 32)) // n) for i in range(n + 1)] if n <= 4096 else None
    if edges is None:                                                  # ceil(i 2^32 / n) without leaving uint64: i 2^32 < 2^52
        i = np.arange(n + 1, dtype=np.uint64)
        e = ((i << np.uint64(32)) + np.uint64(n - 1)) // np.uint64(n)
    else:
        e = np.array(edges, dtype=np.uint64)
    mass = e[1:] - e[:-1]                                              # sums to 2^32
    thresh = t[:, 0].astype(np.uint64)
    alias = np.minimum(t[:, 1].astype(np.int64), n - 1)
    rest = np.uint64(1 << 32) - thresh                                 # 1 .. 2^32
    # mass * share < 2^64 may not fit and the sums certainly do not: carry the high and low 16 bits of the share apart
    hi = np.zeros(n, dtype=np.uint64)
    lo = np.zeros(n, dtype=np.uint64)
    own = np.arange(n)
    for idx, share in ((own, thresh), (alias, rest)):
        np.add.at(hi, idx, mass * (share >> np.uint64(16)))
        np.add.at(lo, idx, mass * (share & np.uint64(0xFFFF)))
    if exact:
        return [(int(h) << 16) + int(l) for h, l in zip(hi.tolist(), lo.tolist())]
    return hi.astype(np.float64) / float(1 << 48) + lo.astype(np.float64) / float(1 << 64)


def sample_negatives(excl, n_item, counts, seed=1, round=0, check=True, total=None, alias=None):
    """mvin_sample_negatives: for every user u, ``counts[u]`` items outside u's exclusion row, uniformly and without
    replacement, as a pure function of (``seed``, ``round``) -- include/mvin_hip.h states the rule.  ``excl``: an
    ``interaction_csr`` pair on the device, or None for no exclusions.  ``counts``: int array [nU], device or host.
    ``alias`` = (tab, mask) of ``alias_table`` (numpy or tensors; ``mask`` may be None) routes the call to
    mvin_sample_negatives_weighted: the draws follow the table's distribution and masked items are ineligible for every
    user; None is the uniform call.
    Returns (neg_ptr int64 [nU+1] = the cumulative counts, neg_items int32 [neg_ptr[-1]]) on the device; user u's negatives
    are neg_items[neg_ptr[u]:neg_ptr[u+1]] in draw order.  A user with fewer eligible items than ``counts[u]`` keeps -1 in
    the slots that cannot be filled:
      check=True   reads the two status words back (one synchronisation) and raises ValueError naming how many users fell
                   short and the first such user's m and c;
      check=False  returns the status tensor (int64 [2]: users short, slots at -1) as a third value and never synchronises,
                   provided ``counts`` is a host array or ``total`` = sum(counts) is passed (sizing the output from device
                   counts is a read-back)."""
    lib = _lib.load()
    if torch.is_tensor(counts) and counts.is_cuda:
        dev = counts.device
        cnt = counts.to(torch.int32).contiguous()
    else:
        host = np.ascontiguousarray(np.asarray(counts.cpu() if torch.is_tensor(counts) else counts, dtype=np.int64))
        if host.size and (host.min() < 0 or host.max() >= (1 << 31)):
            raise ValueError("sample_negatives: counts must lie in [0, 2^31)")
        dev = excl[0].device if excl is not None else torch.device("cuda")
        cnt = torch.from_numpy(host.astype(np.int32)).to(dev)
        if total is None:
            total = int(host.sum())
    n_user = cnt.shape[0]
    neg_ptr = torch.zeros(n_user + 1, dtype=torch.int64, device=dev)
    neg_ptr[1:] = torch.cumsum(cnt, 0)
    if total is None:
        total = int(neg_ptr[-1])
    items = torch.empty(int(total), dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    if total > 0:
        ep, ei = (None, None) if excl is None else (excl[0].contiguous(), excl[1].contiguous())
        if ep is not None and (ep.dtype != torch.int64 or ei.dtype != torch.int32 or ep.shape[0] != n_user + 1):
            raise ValueError("sample_negatives: excl = (ptr int64 [nU+1], ids int32)")
        if ei is not None and ei.numel() == 0:      # nobody excludes anything: an empty tensor has no address to pass
            ep, ei = None, None
        if alias is None:
            _lib.check(lib.mvin_sample_negatives(_p(ep), _p(ei), _p(cnt), _p(neg_ptr), n_user, int(n_item),
                                                 int(seed) & ((1 << 64) - 1), int(round) & ((1 << 64) - 1), _p(items), _p(status),
                                                 _stream()), "mvin_sample_negatives")
        else:
            tab, mask = _alias_on(alias, int(n_item), dev)
            _lib.check(lib.mvin_sample_negatives_weighted(_p(ep), _p(ei), _p(cnt), _p(neg_ptr), n_user, int(n_item), _p(tab),
                                                          _p(mask), int(seed) & ((1 << 64) - 1), int(round) & ((1 << 64) - 1),
                                                          _p(items), _p(status), _stream()), "mvin_sample_negatives_weighted")
    if not check:
        return neg_ptr, items, status
    short_users, short_slots = status.cpu().tolist()
    if short_users:
        u = int(torch.searchsorted(neg_ptr, torch.nonzero(items < 0)[0], right=True)[0]) - 1
        row = np.zeros(0, dtype=np.int64) if excl is None else excl[1][int(excl[0][u]):int(excl[0][u + 1])].cpu().numpy()
        taken = np.zeros(int(n_item), dtype=bool)
        taken[row[(row >= 0) & (row < n_item)]] = True
        if alias is not None and alias[1] is not None:
            mask = np.asarray(alias[1].cpu() if torch.is_tensor(alias[1]) else alias[1]).astype(np.int64).reshape(-1)
            taken |= ((mask[:, None] >> np.arange(32)[None, :]) & 1).astype(bool).reshape(-1)[:int(n_item)]
        c = int(n_item) - int(taken.sum())
        raise ValueError(f"sample_negatives: {short_users} users fell short ({short_slots} slots left at -1); the first is user "
                         f"{u} with m={int(cnt[u])} requested and c={c} eligible items of {int(n_item)}")
    return neg_ptr, items


def _alias_on(alias, n_item, dev):
    """(tab, mask) of ``alias_table`` as contiguous device tensors holding the table's 32-bit words (mask None stays None)."""
    def words(a, shape, what):
        if a is None:
            return None
        if not torch.is_tensor(a):
            a = np.ascontiguousarray(np.asarray(a))
            if a.dtype not in (np.uint32, np.int32):
                raise ValueError(f"sample_negatives: alias {what} must hold 32-bit words, got {a.dtype}")
            a = torch.from_numpy(a.view(np.int32))
        elif a.dtype not in (torch.int32, torch.uint32):
            raise ValueError(f"sample_negatives: alias {what} must hold 32-bit words, got {a.dtype}")
        if tuple(a.shape) != shape:
            raise ValueError(f"sample_negatives: alias {what} of shape {tuple(a.shape)}, expected {shape}")
        return a.to(dev).contiguous()
    tab, mask = alias
    return words(tab, (n_item, 2), "table"), words(mask, ((n_item + 31) // 32,), "mask")


class NegativeSampler(object):
    """Fresh training negatives for every epoch: convert_rating's rule (KGCN/preprocess.py:60-70 -- per user, as many unwatched
    items as positives, without replacement) with the draws made on the device by ``sample_negatives``.

    Holds on ``device``: the positive rows of ``train_data`` (label 1, in ``train_data`` order), the exclusion CSR over the
    label-1 items of ``train_data`` and of every array in ``exclude`` (pass the eval and test splits: no held-out positive is
    then taught as a negative), and the counts m[u] = floor(ratio * p_u + 0.5) with p_u = positives of u in ``train_data``
    (round half up, computed in float64; ``ratio=1.0`` is the reference's ``size=len(pos_item_set)``).  A user with fewer
    eligible items c_u = n_item - |distinct in-range exclusions| than m[u] gets m[u] = c_u; that is said once through
    ``warnings.warn``.  ``epoch(round)`` is a pure function of (seed, round).

    ``dist``: "uniform" draws uniformly over the eligible items (mvin_sample_negatives); "popularity" draws in proportion to
    w_i = (count_i + smooth) ** alpha in float64 (``alpha`` around 0.75 is word2vec's choice), count_i = the label-1 rows of
    ``train_data`` with item i -- never of the ``exclude`` splits, which would leak the held-out sets -- through an alias table
    (``alias_table``, mvin_sample_negatives_weighted).  ``weights``: an explicit array [n_item], which overrides.  An item of
    weight zero is masked: ineligible for every user, and c_u counts it out.  ``draw(round)`` is the one place the negatives
    of a round come from: ``epoch``, ``rank_groups`` and ``hard_groups`` go through it and so follow the distribution."""

    def __init__(self, train_data, n_user, n_item, exclude=(), ratio=1.0, seed=1, device="cuda", dist="uniform", alpha=0.75,
                 smooth=0.0, weights=None):
        if dist not in ("uniform", "popularity"):
            raise ValueError(f"NegativeSampler: dist={dist!r}: expected 'uniform' or 'popularity'")
        d = np.asarray(train_data, dtype=np.int64).reshape(-1, 3)
        pos = d[d[:, 2] == 1]
        self.n_user, self.n_item, self.seed, self.ratio = int(n_user), int(n_item), int(seed), float(ratio)
        self.device = torch.device(device)
        self.pos_rows = torch.from_numpy(np.ascontiguousarray(pos)).to(self.device)
        ptr, ids = _interaction_csr_host([d] + [np.asarray(e) for e in exclude], self.n_user, labels=1)
        self.excl = (torch.from_numpy(ptr).to(self.device), torch.from_numpy(ids).to(self.device))
        n_pos_of = np.bincount(pos[:, 0], minlength=self.n_user).astype(np.int64)
        want = np.floor(self.ratio * n_pos_of.astype(np.float64) + 0.5).astype(np.int64)
        in_range = (ids >= 0) & (ids < self.n_item)
        row_of = np.repeat(np.arange(self.n_user), np.diff(ptr))
        self.dist, self.alias, masked = dist, None, None
        if weights is not None or dist == "popularity":
            if weights is None:
                if not (np.isfinite(alpha) and np.isfinite(smooth) and smooth >= 0):
                    raise ValueError(f"NegativeSampler: alpha={alpha!r}, smooth={smooth!r}: expected finite numbers, smooth >= 0")
                item = pos[:, 1]
                count = np.bincount(item[(item >= 0) & (item < self.n_item)], minlength=self.n_item).astype(np.float64)
                weights = (count + float(smooth)) ** float(alpha)
            tab, mask = alias_table(weights, self.n_item)
            self.alias = _alias_on((tab, mask), self.n_item, self.device)
            self._alias_tab_host = tab
            masked = ((mask[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)[:self.n_item]
            in_range[in_range] = ~masked[ids[in_range]]                # a masked item of the row is counted once, by the mask
        eligible = self.n_item - np.bincount(row_of[in_range], minlength=self.n_user).astype(np.int64)
        if masked is not None:
            eligible -= int(masked.sum())
        m = np.minimum(want, eligible)
        # what log_proposal needs, on the host: c_u, the masked items and the (user, item) pairs the exclusion rows take out
        self.eligible_host = eligible
        self._masked_host = masked
        self._excl_pairs_host = (row_of[in_range], ids[in_range].astype(np.int64))
        self._log_proposal = None
        self.clipped_users = int(np.count_nonzero(want > eligible))
        if self.clipped_users:
            import warnings
            warnings.warn(f"NegativeSampler: {self.clipped_users} users have fewer eligible items than requested negatives; "
                          f"they get every eligible item ({int((want - m).sum())} negatives fewer in all)")
        self.counts_host = m
        self.n_pos, self.n_neg = int(pos.shape[0]), int(m.sum())
        self.counts = torch.from_numpy(m.astype(np.int32)).to(self.device)
        self.neg_users = torch.from_numpy(np.repeat(np.arange(self.n_user, dtype=np.int64), m)).to(self.device)
        # pos_index[i]: the place of positive i among its user's positives, in train_data order (rank_groups hands positive
        # number j of a user the j-th block of the user's negatives)
        order = np.argsort(pos[:, 0], kind="stable")
        first = np.concatenate([[0], np.cumsum(n_pos_of)[:-1]]) if self.n_user else np.zeros(0, dtype=np.int64)
        idx = np.empty(pos.shape[0], dtype=np.int64)
        idx[order] = np.arange(pos.shape[0], dtype=np.int64) - first[pos[order, 0]]
        self.pos_index = torch.from_numpy(idx).to(self.device)
        self.last_status = None

    def log_proposal(self):
        """The log of the proposal the negatives are drawn from, (item_logp float32 [n_item], user_logmass float32 [n_user])
        on the device; computed once, on the host, in float64, and cached.
          item_logp[i]    = log p_i, p_i the probability with which ONE draw produces item i before any exclusion:
                            1 / n_item for the uniform sampler, ``alias_probabilities(tab)`` for a weighted one -- the table's
                            integers, not the float weights it was built from.  A masked item has p_i = 0 and -inf here; it is
                            never drawn, so no valid slot ever looks it up.
          user_logmass[u] = log of the sum of p_i over the items eligible for u: the catalogue minus the distinct in-range ids
                            of u's exclusion row and minus the masked items (-inf for a user with no eligible item, who has
                            no negatives either).
        p_i / user_mass_u is q_u(i), the proposal of one draw conditioned on eligibility (``rank_offsets``)."""
        if self._log_proposal is None:
            if self.alias is None:
                p = np.full(self.n_item, 1.0 / self.n_item, dtype=np.float64)
            else:
                p = alias_probabilities(self._alias_tab_host)
                p[self._masked_host] = 0.0
            rows, ids = self._excl_pairs_host
            mass = p.sum() - np.bincount(rows, weights=p[ids], minlength=self.n_user)
            mass[self.eligible_host <= 0] = 0.0
            with np.errstate(divide="ignore"):
                logs = (np.log(p), np.log(np.maximum(mass, 0.0)))
            self._log_proposal64 = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(self.device) for t in logs)
            self._log_proposal = tuple(t.to(torch.float32) for t in self._log_proposal64)
        return self._log_proposal

    def draw(self, round):
        """(neg_ptr int64 [nU+1], neg_items int32) of ``round`` on the device, from the sampler's distribution (uniform, or the
        alias table's); ``last_status`` keeps the call's status tensor.  Nothing goes back to the host."""
        kw = {} if self.alias is None else {"alias": self.alias}
        neg_ptr, items, self.last_status = sample_negatives(self.excl, self.n_item, self.counts, seed=self.seed, round=round,
                                                            check=False, total=self.n_neg, **kw)
        return neg_ptr, items

    def epoch(self, round):
        """int64 [n_pos + n_neg, 3] (user, item, label) on the device: the positives first, in ``train_data`` order, then the
        negatives of ``round`` (label 0), user-major, each user's in draw order.  Nothing goes back to the host;
        ``last_status`` keeps the call's status tensor."""
        _, items = self.draw(round)
        rows = torch.empty((self.n_pos + self.n_neg, 3), dtype=torch.int64, device=self.device)
        rows[:self.n_pos] = self.pos_rows
        neg = rows[self.n_pos:]
        neg[:, 0] = self.neg_users
        neg[:, 1] = items
        neg[:, 2] = 0
        return rows


def rank_groups(sampler, round):
    """The groups a ranking objective trains on (training.Trainer.set_objective): one group per positive of ``sampler``, a
    ``NegativeSampler`` built with ``ratio`` = n_neg (an integer, 1..63), G = 1 + n_neg slots each.  Returns
    (users int64 [n_pos], items int64 [n_pos, G], valid float32 [n_pos, G]) on the sampler's device, in ``train_data`` order;
    nothing goes to the host.
      slot 0         the positive item;
      slots 1..n_neg positive number j of user u (``sampler.pos_index``) takes entries j*n_neg .. j*n_neg + n_neg - 1 of u's
                     negative row of ``round`` (``sampler.draw``: distinct items, none in the exclusion row), so no two
                     positives of a user share a negative;
      invalid slot   one that lies beyond the user's m[u] (the sampler clipped the row) or holds -1: ``valid`` is 0 there and
                     the slot carries the group's POSITIVE item id -- a valid id for every gather; a masked slot receives no
                     gradient.
    A pure function of (sampler.seed, round)."""
    n_neg = int(sampler.ratio)
    if n_neg != sampler.ratio or not 1 <= n_neg <= 63:
        raise ValueError(f"rank_groups: the sampler's ratio={sampler.ratio!r} must be an integer n_neg in [1, 63]")
    neg_ptr, neg_items = sampler.draw(round)
    dev = sampler.device
    users, pos_item = sampler.pos_rows[:, 0].contiguous(), sampler.pos_rows[:, 1:2]
    k = sampler.pos_index[:, None] * n_neg + torch.arange(n_neg, dtype=torch.int64, device=dev)[None, :]
    ok = k < sampler.counts.to(torch.int64)[users][:, None]                     # inside the user's (possibly clipped) row
    if sampler.n_neg > 0:
        neg = neg_items.to(torch.int64)[(neg_ptr[users][:, None] + k).clamp_(max=sampler.n_neg - 1)]
        ok &= neg >= 0
        neg = torch.where(ok, neg, pos_item.expand(-1, n_neg))
    else:
        neg = pos_item.expand(-1, n_neg)
    items = torch.cat([pos_item, neg], dim=1).contiguous()
    valid = torch.cat([torch.ones_like(pos_item, dtype=torch.float32), ok.to(torch.float32)], dim=1).contiguous()
    return users, items, valid


def candidate_groups(sampler, round, n_neg):
    """The groups of sampled-candidate evaluation (harness.sampled_rank_eval): one group of G = 1 + ``n_neg`` slots per positive
    of ``sampler``, a ``NegativeSampler`` built over the split being evaluated with ``ratio`` = n_neg (an integer, 1..4095)
    and every other split, train included, in ``exclude``.  Returns (users int64 [n_pos], items int64 [n_pos, G], ids int32
    [n_pos, G], slot int32 [n_pos]) on the sampler's device, in the split's order.
      negatives  assigned as ``rank_groups`` assigns them: positive number j of user u (``sampler.pos_index``) takes entries
                 j*n_neg .. j*n_neg + n_neg - 1 of u's negative row of ``round``, in draw order;
      slot       where the positive sits in its group: ``np.random.default_rng([seed, round]).integers(0, G, n_pos)[i]``, drawn
                 once on the host.  NOT slot 0: ties rank the lower position first, so a positive at slot 0 would win every
                 tie and a model whose scores saturate would show a hit ratio of 1.  The negatives fill the other slots in
                 their order;
      ids        the item id of every slot, -1 where the sampler could not fill it (beyond the user's clipped row, or a -1 of
                 the draw): mvin_rank_segments counts no such slot;
      items      what is scored: ``ids`` with the group's positive item in place of every -1, a valid id for every gather.
    A pure function of (sampler.seed, round)."""
    n_neg = int(n_neg)
    if not 1 <= n_neg <= 4095 or sampler.ratio != n_neg:
        raise ValueError(f"candidate_groups: n_neg={n_neg} must lie in [1, 4095] and equal the sampler's ratio={sampler.ratio!r}")
    G = 1 + n_neg
    neg_ptr, neg_items = sampler.draw(round)
    dev = sampler.device
    users, pos_item = sampler.pos_rows[:, 0].contiguous(), sampler.pos_rows[:, 1:2]
    n_pos = users.shape[0]
    k = sampler.pos_index[:, None] * n_neg + torch.arange(n_neg, dtype=torch.int64, device=dev)[None, :]
    ok = k < sampler.counts.to(torch.int64)[users][:, None]                     # inside the user's (possibly clipped) row
    if sampler.n_neg > 0:
        neg = neg_items.to(torch.int64)[(neg_ptr[users][:, None] + k).clamp_(max=sampler.n_neg - 1)]
        neg = torch.where(ok & (neg >= 0), neg, torch.full_like(neg, -1))
    else:
        neg = torch.full((n_pos, n_neg), -1, dtype=torch.int64, device=dev)
    slot = torch.from_numpy(np.random.default_rng([sampler.seed, int(round)]).integers(0, G, n_pos).astype(np.int64)).to(dev)
    col = torch.arange(G, dtype=torch.int64, device=dev)[None, :]
    src = (col - (col > slot[:, None]).to(torch.int64)).clamp_(max=n_neg - 1)   # slot c holds negative c, or c - 1 past the positive
    ids = torch.where(col == slot[:, None], pos_item.expand(-1, G), neg.gather(1, src))
    items = torch.where(ids >= 0, ids, pos_item.expand(-1, G)).contiguous()
    return users, items, ids.to(torch.int32).contiguous(), slot.to(torch.int32)


def rank_offsets(sampler, users, items, valid):
    """The logit offsets of the logQ-corrected sampled softmax (mvin_rank_head_offset, Trainer.set_objective(offset=True)) for
    the groups ``users`` int64 [n] / ``items`` int64 [n, G] / ``valid`` f32 [n, G] of ``rank_groups(sampler, .)`` or a row
    subset of it.  Returns float32 [n, G] on the sampler's device; nothing goes to the host.
      slot 0            0: the positive is in its group with probability 1 and stays uncorrected;
      an invalid slot   0 (the head never reads it);
      a valid negative  log(n_g * p_item / user_mass_u): n_g = the valid negatives of the group, p and user_mass those of
                        ``sampler.log_proposal()``.  log n_g + log p - log user_mass is evaluated in float64 (from the float64
                        logs the sampler caches beside the float32 pair) and rounded once to float32.
    With these offsets the group's softmax denominator is the importance-sampling estimate
        Z ~ exp(s_0) + (1 / n_g) sum_j exp(s_j) / q_u(j),   q_u(j) = p_j / user_mass_u,
    of the partition function over ALL of the user's eligible items plus the positive (Bengio & Senecal's sampled softmax;
    the "logQ correction" of Yi et al. 2019), under a uniform proposal as much as under a popularity-weighted one.
    An approximation, the usual practice, not exact: q_u is the proposal of ONE draw conditioned on eligibility.  The sampler
    draws a user's negatives WITHOUT replacement, and all of that user's positives take theirs from one shared row, so the
    true inclusion probability of an item differs from n_g * q_u by terms of order m_u * max q (m_u the user's negatives of
    the epoch)."""
    sampler.log_proposal()
    logp, logmass = sampler._log_proposal64
    neg = valid != 0
    neg[:, 0] = False
    n_g = neg.sum(dim=1, keepdim=True).to(torch.float64)
    c = torch.log(n_g) + logp[items] - logmass[users][:, None]
    return torch.where(neg, c, torch.zeros_like(c)).to(torch.float32).contiguous()


def select_negatives(*args, **kwargs):
    """ops.select_negatives (mvin_select_negatives), bound late: ``hard_groups`` reaches the kernel through this name."""
    from . import ops
    return ops.select_negatives(*args, **kwargs)


def hard_groups(sampler, round, scores, n_neg, shortlist, group_key=None, counts=None, pool=None):
    """The groups a ranking objective trains on under ``negatives="hard"``: out of the POOL groups of ``sampler`` -- a
    ``NegativeSampler`` built with ``ratio`` = M, the pool size, ``rank_groups(sampler, round)``: one positive and up to M
    distinct unwatched items of its user -- and the current model's ``scores`` of every pool slot (f32 [n, 1 + M]), the
    ``n_neg`` negatives per positive that mvin_select_negatives picks: uniform among the ``shortlist`` highest-scored valid
    candidates (include/mvin_hip.h states the rule; ``shortlist == n_neg``: the hardest, ``shortlist == M``: uniform whatever
    the scores).  ``pool``: the (users, items, valid) of ``rank_groups(sampler, round)`` or a row subset of it, when the caller
    holds it already (None: drawn here); ``group_key`` int64 [n]: each row's index in ``train_data`` order (None: row g is
    positive g), the key of the row's random draw, so that a row's result does not depend on where it stands.
    Returns (users int64 [n], items int64 [n, 1 + n_neg], valid f32 [n, 1 + n_neg]) in the layout of ``rank_groups``, the chosen
    negatives hardest first; ``counts`` (int64 [4]) accumulates the integers of "hard_rate" / "pool_rate".  A pure function of
    (sampler.seed, round, scores); nothing goes to the host."""
    M = int(sampler.ratio)
    n_neg, shortlist = int(n_neg), int(shortlist)
    if M != sampler.ratio or not 1 <= M <= 63:
        raise ValueError(f"hard_groups: the sampler's ratio={sampler.ratio!r} must be an integer pool size in [1, 63]")
    if not 1 <= n_neg <= M:
        raise ValueError(f"hard_groups: n_neg={n_neg} must lie in [1, pool = {M}]")
    if not n_neg <= shortlist <= M:
        raise ValueError(f"hard_groups: shortlist={shortlist} must lie in [n_neg = {n_neg}, pool = {M}]")
    users, items, valid = rank_groups(sampler, round) if pool is None else pool
    if tuple(scores.shape) != tuple(items.shape):
        raise ValueError(f"hard_groups: scores {tuple(scores.shape)} for pool groups {tuple(items.shape)}")
    out_items, out_valid = select_negatives(scores, items, valid, n_neg, shortlist, sampler.seed, round, group_key=group_key,
                                            counts=counts)
    return users, out_items, out_valid


# --------------------------------------------------------------------------- KG exploration
def kg_edge_index(csr):
    """The DISTINCT edges of a ``build_csr`` KG as (eptr int64 [nE+1], edst int32 [M], erel int32 [M]) on its device: row h =
    the distinct (tail, relation) pairs listed under h, ascending by (tail, relation).  Duplicate CSR slots of one row count
    once, as in the reference's ``set`` of (h, t, r) tuples (data_loader_user_set.py:208-239).  Host plumbing (torch unique),
    like ``build_csr``."""
    indptr, dst, rel = csr
    n_entity = indptr.shape[0] - 1
    dev = indptr.device
    if dst.numel() == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return torch.zeros(n_entity + 1, dtype=torch.int64, device=dev), z, z.clone()
    src = torch.repeat_interleave(torch.arange(n_entity, device=dev), indptr[1:] - indptr[:-1])
    rows = torch.unique(torch.stack([src, dst.long(), rel.long()], dim=1), dim=0)          # lexicographic, distinct
    eptr = torch.zeros(n_entity + 1, dtype=torch.int64, device=dev)
    eptr[1:] = torch.cumsum(torch.bincount(rows[:, 0], minlength=n_entity), 0)
    return eptr.contiguous(), rows[:, 1].to(torch.int32).contiguous(), rows[:, 2].to(torch.int32).contiguous()


class KGExploration(object):
    """How much of the KG within the model's reach the sampled adjacencies have covered so far (the reference's
    get_all_user_entity_count -> args.use_neighbor_rate = [all, used, rate], data_loader_user_set.py:208-239, which it leaves
    commented out and returns [0, 0, 0] for).

    ``seeds``: the items of train_data[:, 1] under any label (the reference's item_pool); repeats are fine.  ``hops``: pass
    ``config.tree_depth(args)`` = n_mix_hop * h_hop, the depth the model actually reads -- the reference passes ``h_hop``,
    which is the same thing at n_mix_hop = 1.  The FIELD is every distinct edge (h, t, r) whose head lies in F_i for some
    i < hops, with F_0 = seeds and F_{i+1} = the tails of the edges leaving F_i (it replaces F_i, as in the reference).
    ``update`` walks one adjacency the same way from the seeds, but follows a slot (h, adj_entity[h,k], adj_relation[h,k]) only
    when it is an edge of the KG (the all-zero row of an entity without edges is not), so explored is a subset of the field and
    ``rate`` never exceeds 1.  Everything is an exact integer count made on the device (ops.kg_field / ops.kg_explore)."""

    def __init__(self, csr, seeds, hops):
        from . import ops
        self.index = kg_edge_index(csr)
        dev = self.index[0].device
        self.n_entity, self.n_edges, self.hops = self.index[0].shape[0] - 1, self.index[1].numel(), int(hops)
        s = seeds if torch.is_tensor(seeds) else torch.from_numpy(np.unique(np.asarray(seeds, dtype=np.int64)))
        s = s.to(dev).reshape(-1)
        s = s[(s >= 0) & (s < self.n_entity)]       # ids beyond int32 cannot be entities; the kernels ignore the rest themselves
        self.seeds = s.to(torch.int32).contiguous()
        self.field_bits, counts = ops.kg_field(self.index, self.seeds, self.hops)
        counts = counts.cpu().tolist()
        self.frontier_sizes, self.field_edges = counts[:-1], int(counts[-1])
        self.explored_bits = torch.zeros_like(self.field_bits)
        self.explored_total, self.n_updates = 0, 0

    def update(self, adj_entity, adj_relation):
        """Add one sampled adjacency (device tensors, or numpy arrays as MVIN.set_adjacency takes them).  Returns
        (explored_now, new, explored_total): edges this adjacency reaches, those no earlier one had reached, all so far."""
        from . import ops
        dev = self.index[0].device

        def conv(a):
            if torch.is_tensor(a):
                return a.to(dev).to(torch.int32).contiguous()
            return torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev).contiguous()
        now, new, total = ops.kg_explore(self.index, conv(adj_entity), conv(adj_relation), self.seeds, self.hops,
                                         self.explored_bits).cpu().tolist()
        self.explored_total, self.n_updates = int(total), self.n_updates + 1
        return int(now), int(new), int(total)

    @property
    def rate(self):
        return self.explored_total / self.field_edges if self.field_edges else 0.0
