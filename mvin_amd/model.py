"""MVIN model -- the reference's call surface (src/model/MVIN/model.py:6-444) on top of
libmvin_hip.so.  Host code in Python on PyTorch-ROCm (device memory + stream only); every
op of the scoring path is a hand-written gfx950 kernel reached through the C ABI.

    model = MVIN(args, n_user, n_entity, n_relation, adj_entity, adj_relation)
    model.get_scores(sess, feed_dict) -> (item_indices, sigmoid_scores)     model.py:443-444
    model.eval(sess, feed_dict)       -> (auc, acc, f1)                      model.py:419-426
    model.eval_case_study(sess, feed) -> 7-tuple                             model.py:428-441
    model.train(sess, feed_dict)      -> (None, loss)                        model.py:416-417

``sess`` is accepted and ignored (there is no TF session); feed keys are the placeholder
sentinels ``model.user_indices / item_indices / labels / memories_{h,r,t}[i]``
(train.py:113-120, util.py:209-230).  Unlike the reference graph, whose static reshapes
bake ``batch_size`` in (model.py:251,281,296), any batch length is accepted.

How the forward is arranged (see DESIGN.md for the data layout and the kernel roofline):
  * ids of levels 0..L-1 are expanded on device (mvin_expand_ids); level L is never
    materialised -- the deepest aggregator hop reads the adjacency rows itself and gathers
    the K^L entity rows straight into a wave-level softmax / weighted sum
    (mvin_gather_attn_fwd);
  * the user-oriented projection (model.py:270-283) is applied AFTER the weighted sum on
    the deepest level ((sum_k p_k E[y_k]).W + c == sum_k p_k (E[y_k].W + c) as sum_k p_k = 1)
    and per row on the small upper levels (mvin_linear_fwd with a gathered source);
  * attention logits use the nR-entry table t[r] = Rel[r].urh_w[D:2D]: the user and self
    terms of aggregators.py:130-133 are constant over k and cancel in the softmax;
  * key addressing (model.py:161-240) uses (R h).v == h.(v R): V[b,r,:] = E[item_b].R_KGE[r]
    is computed once per pair, then each memory needs one D-long dot product.
"""
import os
import weakref
from types import SimpleNamespace

import numpy as np
import torch

from . import l2_plan, ops, route_plan
from .aggregators import SumAggregator_urh_matrix
from .params import aggregator_keys, init_params


class Placeholder(object):
    """Hashable stand-in for a tf.placeholder used as a feed_dict key (model.py:49-64)."""

    def __init__(self, name, dtype, shape):
        self.name, self.dtype, self.shape = name, dtype, shape

    def __repr__(self):
        return f"<Placeholder {self.name} {self.dtype} {self.shape}>"


class _SmallOut(object):
    """Results of the single-launch pass: one device buffer [user_o | item_embeddings | scores | sigmoid scores]; the four
    tensors are views created on access (same attribute names as the namespace the other schedules return)."""
    __slots__ = ("_buf", "_B", "_D", "importance_list")

    def __init__(self, buf, B, D):
        self._buf, self._B, self._D, self.importance_list = buf, B, D, []

    @property
    def user_o(self):
        return self._buf[:self._B * self._D].view(self._B, self._D)

    @property
    def item_embeddings(self):
        n = self._B * self._D
        return self._buf[n:2 * n].view(self._B, self._D)

    @property
    def scores(self):
        n = 2 * self._B * self._D
        return self._buf[n:n + self._B]

    @property
    def scores_normalized(self):
        n = 2 * self._B * self._D + self._B
        return self._buf[n:n + self._B]


class MVIN(object):
    def __init__(self, args, n_user, n_entity, n_relation, adj_entity, adj_relation,
                 params=None, device=None, seed=0, fused=None, table_dtype="f32", hoist=False):
        """``table_dtype="bf16"`` keeps the entity embedding table in bf16 (BASELINE config C5):
        rows are widened to fp32 inside the kernels, all arithmetic stays fp32; scoring only.
        ``hoist``: entity-table mode of the two deepest levels (see ``hoist_entity_tables``):
        False = off (the faithful per-pair gather), True = per-entity tables cached until a
        parameter / the adjacency changes, "step" = rebuilt inside every forward."""
        self.device = torch.device(device or "cuda")
        if table_dtype not in ("f32", "bf16"):
            raise ValueError("table_dtype must be 'f32' or 'bf16'")
        self.table_dtype = table_dtype
        # fused=False (or MVIN_FUSED=0) forces the per-level kernels (used by the tests to
        # check both HIP paths against the oracle)
        self.fused = (os.environ.get("MVIN_FUSED", "1") != "0") if fused is None else bool(fused)
        if hoist not in (False, True, "step"):
            raise ValueError("hoist must be False, True or 'step'")
        self.hoist = hoist
        self.dedup = None            # None: MVIN_L2_ENC / auto; True / False: force the encoded / the plain adjacency
        self._l2_static, self._l2_memo = None, {}             # see _l2_shape_caps, _l2_plan
        self._route_static, self._route_memo = None, {}       # see _route_inputs, _route
        self._hoisted = None
        self._table_token = None     # see _hoist_key
        self._parse_args(args, adj_entity, adj_relation)
        self._build_inputs()
        self._build_model(n_user, n_entity, n_relation, params, seed)
        self._build_train()
        self._built = True
        self.prepare()

    # ------------------------------------------------------------------ construction
    def _parse_args(self, args, adj_entity, adj_relation):
        """model.py:17-47."""
        self.dataset = getattr(args, "dataset", None)
        self.load_pretrain_emb = getattr(args, "load_pretrain_emb", False)
        self.h_hop = args.h_hop
        self.batch_size = args.batch_size
        self.n_neighbor = args.neighbor_sample_size
        self.p_hop = args.p_hop
        self.dim = args.dim
        self.l2_weight = getattr(args, "l2_weight", 0.0)
        self.l2_agg_weight = getattr(args, "l2_agg_weight", 0.0)
        self.kge_weight = getattr(args, "kge_weight", 0.0)
        self.lr = getattr(args, "lr", 0.0)
        self.save_model_name = getattr(args, "save_model_name", "model1")
        self.n_mix_hop = args.n_mix_hop
        self.n_memory = args.n_memory
        self.update_item_emb = getattr(args, "update_item_emb", None)
        self.h0_att = getattr(args, "h0_att", None)
        self.path = getattr(args, "path", None)
        self.User_orient_rela = bool(args.User_orient_rela)
        self.args = args
        self.aggregator_class = SumAggregator_urh_matrix
        self.agg_fun = self.aggregate_delta_whole if args.wide_deep else self.aggregate
        if self.dim % 4 != 0 or not (4 <= self.dim <= 256):
            raise ValueError("dim must be a multiple of 4 in [4, 256] (16-byte row loads)")
        if tuple(adj_entity.shape) != tuple(adj_relation.shape) or adj_entity.shape[1] != self.n_neighbor:
            raise ValueError("adj_entity/adj_relation must both be [n_entity, neighbor_sample_size]")
        self.set_adjacency(adj_entity, adj_relation)

    def set_adjacency(self, adj_entity, adj_relation):
        """Install a (re-)sampled adjacency: numpy int64 arrays as the reference builds them
        (data_loader_user_set.py:377-378) or device tensors from mvin_amd.data_prep.construct_adj.
        Kept as int32 on the device: halves the id traffic (n_entity < 2^31)."""
        def conv(a):
            if isinstance(a, torch.Tensor):
                return a.to(self.device).to(torch.int32).contiguous()
            return torch.from_numpy(np.asarray(a).astype(np.int32)).to(self.device).contiguous()
        self.adj_entity, self.adj_relation = conv(adj_entity), conv(adj_relation)
        self._hoisted = None
        self._enc = None             # duplicate-slot encoding, built on first use (encoded_adjacency)
        self._generation = getattr(self, "_generation", 0) + 1
        if getattr(self, "_built", False):
            self.prepare()           # the encoding of the NEW adjacency, eagerly (never inside a later forward / capture)

    def encoded_adjacency(self):
        """(enc_entity, enc_relation, cnt, mean distinct fraction) of the current adjacency (mvin_encode_adjacency),
        built once per set_adjacency; None when the shape has no packed-tile kernel."""
        if self._enc is None:
            if torch.cuda.is_current_stream_capturing():
                # two launches, an allocation and a host sync (.item()): none of that belongs in a captured graph
                raise RuntimeError("the duplicate-slot encoding of the adjacency is not built yet: call model.prepare() "
                                   "(or run one eager forward) before capturing a graph")
            if not self._l2_shape_caps()[1].enc:
                self._enc = False
            else:
                enc_e, enc_r, cnt = ops.encode_adjacency(self.adj_entity, self.adj_relation)
                frac = float(cnt.float().mean().item()) / self.n_neighbor      # one host sync per adjacency
                self._enc = (enc_e, enc_r, cnt, frac)
        return self._enc or None

    # ------------------------------------------------------------------ form of the two deepest levels (mvin_amd/l2_plan.py)
    # thresholds: l2_plan.THRESHOLDS, each with its measurement; these three stay settable (class or model), read through the table
    ENC_AUTO_MAX_DISTINCT_FRACTION = l2_plan.THRESHOLDS.enc_auto_max_distinct_fraction
    ENC_AUTO_MIN_PARENTS = l2_plan.THRESHOLDS.enc_auto_min_parents
    ITEM_ORDER_MIN_BATCH = l2_plan.THRESHOLDS.item_order_min_batch

    def _enc_mode(self):         # "0" / "1": the plain / the encoded adjacency forced; else automatic
        return os.environ.get("MVIN_L2_ENC", "auto") if self.dedup is None else ("1" if self.dedup else "0")

    def _l2_shape_caps(self):
        """(L2Shape, L2Caps): the shape and the library's capability answers, gathered once per (n_entity, n_relation, dim, K, table dtype)."""
        E = self.entity_emb_matrix
        key = (self.n_entity, self.n_relation, E.dtype, E.numel(), self.fused, self.args.User_orient)
        c = self._l2_static
        if c is None or c[0] != key:
            D, K, nE, nR = self.dim, self.n_neighbor, int(self.n_entity), int(self.n_relation)
            sh = l2_plan.L2Shape(D, K, self.n_mix_hop * self.h_hop, nE, nR, E.dtype == torch.float32, E.numel() * E.element_size(),
                                 bool(self.args.User_orient), self.fused)
            caps = l2_plan.L2Caps(enc=K <= 128 and nR <= 4096 and nE <= (1 << 24) and ops.encode_adjacency_supported(D, K),
                                  prj_plain=ops.gather_attn_l2_prj_supported(D, K, False, nE, nR),
                                  agg=ops.gather_attn_l2_agg_supported(D, K, nE, nR), fold=ops.score_l2_folded_supported(D, K, nE, nR),
                                  fold_gather=ops.score_l2_folded_gather_supported(D, K, nE, nR))
            c = self._l2_static = (key, sh, caps)
        return c[1], c[2]

    def _l2_inputs(self, want_probs=False):
        """(shape, overrides, capabilities, thresholds, distinct fraction) as l2_plan takes them; the mean fraction of distinct slots per
        adjacency row is None without an encoding (which is not built where no call can take it)."""
        sh, caps = self._l2_shape_caps()
        th = l2_plan.THRESHOLDS._replace(enc_auto_max_distinct_fraction=self.ENC_AUTO_MAX_DISTINCT_FRACTION,
                                         enc_auto_min_parents=self.ENC_AUTO_MIN_PARENTS, item_order_min_batch=self.ITEM_ORDER_MIN_BATCH)
        mode = self._enc_mode()
        ov = l2_plan.L2Overrides(self.prj, self.agg, self.fold, mode, self.item_order, os.environ.get("MVIN_L2_WPP", "1") != "0")
        enc = None if (want_probs or self.fused is False or mode == "0") else self.encoded_adjacency()
        return sh, ov, caps, th, None if enc is None else enc[3]

    def _l2_plan(self, B, n_parents, want_probs=False, use_tail=True, gather_form=True):
        # remembered per everything it reads, as raw attributes: ~2 us against ~6.5 for gathering the inputs and deciding (the native
        # call at a few thousand pairs is host-bound)
        E = self.entity_emb_matrix
        key = (B, n_parents, want_probs, use_tail, gather_form, self.prj, self.agg, self.fold, self._enc_mode(), self.item_order, self.fused,
               self._generation, E.dtype, E.numel(), self.n_entity, self.n_relation, self.args.User_orient, os.environ.get("MVIN_L2_WPP"),
               self.ENC_AUTO_MAX_DISTINCT_FRACTION, self.ENC_AUTO_MIN_PARENTS, self.ITEM_ORDER_MIN_BATCH)
        plan = self._l2_memo.get(key)
        if plan is None:
            if len(self._l2_memo) >= 64:
                self._l2_memo.clear()
            plan = self._l2_memo[key] = l2_plan.plan(*self._l2_inputs(want_probs), B, n_parents, want_probs, use_tail, gather_form)
        return plan

    # the plan's rules one by one, as bench.py and the tests read them
    def _enc_for_l2(self, want_probs=False, n_parents=None):
        """The encoded adjacency when the two deepest levels should take the packed-tile kernel for this call."""
        return self.encoded_adjacency() if l2_plan.encoded(*self._l2_inputs(want_probs), n_parents, want_probs) else None

    def _prj_for_l2(self, B, n_parents=None):
        return l2_plan.projected(*self._l2_inputs()[:4], B, n_parents)

    def _prj_plain_ok(self):
        return l2_plan.projected_plain(*self._l2_shape_caps())

    def _agg_for(self, enc):
        _, ov, caps, _, _ = self._l2_inputs()
        return l2_plan.aggregates(ov, caps, enc is not None)

    def _fold_for(self, enc):
        sh, ov, caps, _, _ = self._l2_inputs()
        return l2_plan.folded(sh, ov, caps, enc is not None)

    def _agg_shape_ok(self):
        return bool(self._l2_shape_caps()[1].agg)

    def _fold_shape_ok(self):
        return bool(self._l2_shape_caps()[1].fold)

    def _fold_gather_ok(self):
        return bool(self._l2_shape_caps()[1].fold_gather)

    def _item_order_for(self, B):
        sh, ov, _, th, _ = self._l2_inputs()
        return l2_plan.item_order(sh, ov, th, B)

    def _stream_ws(self, cache, n_ws, dtype=torch.float32, stream=None):
        """The current stream's workspace of ``n_ws`` elements in ``cache`` (a dict per kind, keyed by stream handle); reallocated when n_ws changes."""
        cs = torch.cuda.current_stream().cuda_stream if stream is None else stream
        ws = cache.get(cs)
        if ws is None or ws.numel() != n_ws:
            ws = cache[cs] = torch.empty((n_ws,), dtype=dtype, device=self.device)
        return ws

    def _build_inputs(self):
        """model.py:49-64."""
        self.user_indices = Placeholder("user_indices", "int64", [None])
        self.item_indices = Placeholder("item_indices", "int64", [None])
        self.labels = Placeholder("labels", "float32", [None])
        self.memories_h, self.memories_r, self.memories_t = [], [], []
        for hop in range(max(1, self.p_hop)):
            self.memories_h.append(Placeholder(f"memories_h_{hop}", "int32", [None, self.n_memory]))
            self.memories_r.append(Placeholder(f"memories_r_{hop}", "int32", [None, self.n_memory]))
            self.memories_t.append(Placeholder(f"memories_t_{hop}", "int32", [None, self.n_memory]))

    def _build_model(self, n_user, n_entity, n_relation, params, seed):
        """model.py:69-122 (parameters).  The graph body (:125-159) runs in ``forward_device``."""
        a = self.args
        self.n_user, self.n_entity, self.n_relation = n_user, n_entity, n_relation
        if params is None:
            params = init_params(a, n_user, n_entity, n_relation, seed=seed)
        D, H, M = self.dim, self.h_hop, self.n_mix_hop
        L = M * H

        def dev(x):
            return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(self.device).contiguous()

        self.user_emb_matrix = dev(params["user_emb_matrix"])
        self.entity_emb_matrix = dev(params["entity_emb_matrix"])
        if self.table_dtype == "bf16":
            self.entity_emb_matrix = self.entity_emb_matrix.to(torch.bfloat16).contiguous()
        self.relation_emb_matrix = dev(params["relation_emb_matrix"])
        self.relation_emb_KGE_matrix = dev(params["relation_emb_KGE_matrix"])
        for t, shape in ((self.user_emb_matrix, (n_user, D)), (self.entity_emb_matrix, (n_entity, D)),
                         (self.relation_emb_matrix, (n_relation, D)),
                         (self.relation_emb_KGE_matrix, (n_relation, D, D))):
            if tuple(t.shape) != shape:
                raise ValueError(f"parameter shape {tuple(t.shape)} != {shape}")
        self.enti_transfer_matrix_list = [dev(params[f"enti_transfer_matrix_{n}"]) for n in range(M)]
        self.enti_transfer_bias_list = [dev(params[f"enti_transfer_bias_{n}"]) for n in range(M)]
        self.user_mlp_matrix = dev(params["user_mlp_matrix"])
        self.user_mlp_bias = dev(params["user_mlp_bias"])
        # the L+1 projection matrices live in one stack so q.W_e + b_e for every level is one launch
        self._transfer_W = dev(np.stack([params[f"transfer_matrix_{e}"] for e in range(L + 1)]))
        self._transfer_b = dev(np.stack([params[f"transfer_bias_{e}"] for e in range(L + 1)]))
        self.transfer_matrix_list = [self._transfer_W[e] for e in range(L + 1)]
        self.transfer_matrix_bias = [self._transfer_b[e] for e in range(L + 1)]
        self.transform_matrix, self.transform_bias = self.transfer_matrix_list[-1], self.transfer_matrix_bias[-1]
        self.h_emb_item_mlp_matrix = dev(params["h_emb_item_mlp_matrix"])
        self.h_emb_item_mlp_bias = dev(params["h_emb_item_mlp_bias"])
        # aggregators (model.py:290 / :359)
        self._agg = {}
        self.aggregators = []
        if not a.PS_only:
            for (i, n) in aggregator_keys(a):
                tag = f"agg_{i}_{n}_"
                name = (str(i) + "_" + str(n)) if a.wide_deep else i
                agg = self.aggregator_class(
                    self.save_model_name, self.batch_size, D, name=name,
                    User_orient_rela=(self.User_orient_rela if a.wide_deep else True),
                    weights=params[tag + "weights"], bias=params[tag + "bias"],
                    urh_weights=params[tag + "urh_weights"], urh_bias=params[tag + "urh_bias"],
                    relation_emb=self.relation_emb_matrix, device=self.device)
                self._agg[(i, n)] = agg
                self.aggregators.append(agg)
        self._profile = None
        self._native_l2_state = None
        self._native_l2_ws = {}
        # projected-tables form of the fused two-level pass inside mvin_score_l2_fwd (_prj_for_l2): None = by batch size
        self.prj = {"0": False, "1": True}.get(os.environ.get("MVIN_PRJ", ""), None)
        self._prj_tables = {}                # per stream: workspace of mvin_project_tables_elems floats, rewritten by every call
        # per-entity aggregates S0 | G of those tables (_agg_for): None = whenever the projected-tables form is taken on a shape the
        # kernels take (MVIN_L2_AGG=0 / 1 overrides: 0 answers through the library too)
        self.agg = {"0": False, "1": True}.get(os.environ.get("MVIN_L2_AGG", ""), None)
        self._agg_tables = {}                # per stream: workspace of mvin_entity_aggregates_elems floats, rewritten by every call
        # folded-tail form of the native call (_fold_for): None = whenever the aggregates form is taken (MVIN_L2_FOLD=0 / 1 overrides)
        self.fold = {"0": False, "1": True}.get(os.environ.get("MVIN_L2_FOLD", ""), None)
        self._fold_ws = {}                   # per stream: workspace of mvin_fold_tables_elems floats, rewritten by every call
        # schedule, feed and key-addressing form of a call: mvin_amd/route_plan.py (thresholds and measurements: its THRESHOLDS)
        # gathered form of the grouped key addressing (mvin_key_addressing_grouped_er_fwd): on request only (MVIN_KA_ER=1)
        self.ka_er = os.environ.get("MVIN_KA_ER", "0") == "1"
        self._ka_er_ws = {}                  # per stream: workspace of mvin_project_relations_elems floats, rewritten by every call
        # flash form of the grouped key addressing + user MLP (mvin_key_addressing_flash_fwd): None = automatic (MVIN_KA_FLASH=0 / 1
        # overrides), True / False
        self.ka_flash = {"0": False, "1": True}.get(os.environ.get("MVIN_KA_FLASH", ""), None)
        self._ka_flash_ws = {}               # per stream: workspace of mvin_key_addressing_flash_tables_elems floats, rewritten by every call
        # parents of the projected-tables launch in item order (_item_order_for): None = by batch size (MVIN_ITEM_ORDER=0 / 1 overrides)
        self.item_order = {"0": False, "1": True}.get(os.environ.get("MVIN_ITEM_ORDER", ""), None)
        self._distinct_hint = None           # forward_device's distinct_users of the last call: the default of the _ka_flash_for view
        th = route_plan.THRESHOLDS
        self.group_min_pairs_per_user = th.group_min_pairs_per_user      # batch size / users above which pairs are grouped by user
        self.native_l2_max_batch = th.native_l2_max_batch
        # pairs up to which the whole pass is ONE kernel launch: 0 or MVIN_SMALL=0 turns it off; MVIN_SMALL_MAX overrides
        self.small_max_batch = 0 if os.environ.get("MVIN_SMALL", "1") == "0" else int(os.environ.get("MVIN_SMALL_MAX", th.small_max_batch))
        self.small_group = 0                 # pairs per workgroup of that launch (0: chosen by the library)
        self._small_state = None
        # Device-resident feeds (forward_device / forward_users): ids are NOT validated per batch by default (it costs a
        # host sync; the kernels clamp entity / user / relation ids into their tables instead of reading out of bounds).
        # True (or MVIN_CHECK_IDS=1): every batch is checked and raises IndexError like the host-feed path and like
        # the reference's CPU tf.gather (InvalidArgument).  A user_triplet_set is always checked once, when first seen.
        self.validate_device_ids = os.environ.get("MVIN_CHECK_IDS", "0") == "1"
        self._uts_ok = None
        # grouped key addressing over STATIC per-user records (mvin_build_user_records: relation buckets, tile table, clamped
        # head / tail ids of every user's ripple sets, built once per user_triplet_set tensor): None = where the library has
        # the kernel (MVIN_KA_STATIC=0 turns it off), False = never
        self.static_user_records = None
        self._uts_records = None

    # ------------------------------------------------------------------ schedule, feed, key-addressing form (mvin_amd/route_plan.py)
    # thresholds: route_plan.THRESHOLDS, each with its measurement; the two byte caps stay settable (class or model), read through the table
    USER_RECORDS_MAX_BYTES = route_plan.THRESHOLDS.user_records_max_bytes
    FLASH_TABLES_MAX_BYTES = route_plan.THRESHOLDS.flash_tables_max_bytes

    def _route_shape_caps(self):
        """(RouteShape, RouteCaps): the shape and the library's capability answers, gathered once per (table, adjacency size, fused, hoist)."""
        E = self.entity_emb_matrix
        key = (E.dtype, E.numel(), self.adj_entity.numel(), self.fused, self.hoist, self.n_entity, self.n_relation)
        c = self._route_static
        if c is None or c[0] != key:
            a, D, K, P, Nm, nE, nR = self.args, self.dim, self.n_neighbor, self.p_hop, self.n_memory, int(self.n_entity), int(self.n_relation)
            f32, set_ = E.dtype == torch.float32, 1 if a.PS_O_ft else 0
            sh = route_plan.RouteShape(bool(a.wide_deep), bool(a.PS_only), bool(a.HO_only), bool(a.User_orient_kg_eh), bool(a.PS_O_ft), D, K,
                                       self.h_hop, self.n_mix_hop, P, Nm, nR, nE, f32, E.numel() * E.element_size(),
                                       self.adj_entity.numel() * self.adj_entity.element_size(), bool(self.fused), bool(self.hoist))
            caps = route_plan.RouteCaps(
                score_small=ops.score_small_supported(D, K, P, Nm, nR), l2_tail=ops.l2_tail_supported(D),
                gather_attn_l2=ops.gather_attn_l2_supported(D, K), key_addressing=ops.key_addressing_supported(Nm, D),
                key_addressing_grouped=ops.key_addressing_grouped_supported(D, P, Nm, nR),
                user_records=ops.user_records_supported(D, P, Nm, nR, E.dtype == torch.bfloat16),
                key_addressing_flash=ops.key_addressing_flash_supported(D, P, Nm, nR, nE),
                key_addressing_grouped_er=ops.key_addressing_grouped_er_supported(D, P, Nm, nR, nE, bool(set_)),
                flash_tables_elems=int(ops._lib.load().mvin_key_addressing_flash_tables_elems(nE, nR, D, P, set_)),
                user_records_words=ops.user_records_len(P, Nm, nR))
            c = self._route_static = (key, sh, caps)
        return c[1], c[2]

    def _route_inputs(self):
        """(shape, capabilities, overrides, thresholds) as route_plan takes them."""
        sh, caps = self._route_shape_caps()
        ov = route_plan.RouteOverrides(self.ka_flash, self.ka_er, self.static_user_records, os.environ.get("MVIN_KA_STATIC", "1"),
                                       self.validate_device_ids, self._profile is not None, self.small_max_batch, self.native_l2_max_batch,
                                       self.group_min_pairs_per_user)
        th = route_plan.THRESHOLDS._replace(user_records_max_bytes=self.USER_RECORDS_MAX_BYTES, flash_tables_max_bytes=self.FLASH_TABLES_MAX_BYTES)
        return sh, caps, ov, th

    def _route(self, user, item, mem_h, mem_r, mem_t, uts, want_probs, distinct_users):
        """The route of this call (route_plan.plan), remembered per everything it reads, as raw attributes (as _l2_plan)."""
        B, E, P = item.shape[0], self.entity_emb_matrix, self.p_hop
        if uts is not None:
            fk = (uts.dtype, uts.is_contiguous(), uts.shape, self._records_cached(uts) is not None)
        elif mem_h is None:
            fk = "none"
        elif mem_h[0].dim() == 1:
            fk = "shared"
        else:           # per-pair lists: the first p_hop of each are int32, contiguous, [B, Nm]
            fk, shape, i32 = len(mem_h) >= P and len(mem_r) >= P and len(mem_t) >= P, (B, self.n_memory), torch.int32
            for lst in (mem_h, mem_r, mem_t):
                for m_ in lst[:P]:
                    if m_.dtype != i32 or m_.shape != shape or not m_.is_contiguous():
                        fk = False
        key = (fk, B, item.dtype, user.dtype, user.numel(), want_probs, distinct_users, self._profile is None, self.fused, self.hoist,
               self.ka_flash, self.ka_er, self.static_user_records, os.environ.get("MVIN_KA_STATIC"), self.small_max_batch,
               self.native_l2_max_batch, self.group_min_pairs_per_user, self.USER_RECORDS_MAX_BYTES, self.FLASH_TABLES_MAX_BYTES,
               E.dtype, E.numel(), self._generation)
        route = self._route_memo.get(key)
        if route is None:
            if len(self._route_memo) >= 64:
                self._route_memo.clear()
            sh, caps, ov, th = self._route_inputs()
            kind, i32, cont, shape, n_user, rec_ok = fk if isinstance(fk, str) else "pairs", fk is True, fk is True, fk is True, 0, False
            if uts is not None:
                kind, i32, cont, n_user = "uts", uts.dtype == torch.int32, uts.is_contiguous(), int(uts.shape[0])
                shape = uts.dim() == 4 and uts.shape[1] == max(1, P) and uts.shape[3] == self.n_memory
                rec_ok = uts.is_cuda and self._records_ok(uts, caps)
            fd = route_plan.Feed(kind, B, item.dtype == torch.int64, user.dtype == torch.int64, user.dtype == torch.int32, user.numel(),
                                 i32, cont, shape, n_user, distinct_users, bool(want_probs), rec_ok)
            route = self._route_memo[key] = route_plan.plan(sh, caps, ov, th, fd)
        return route

    def _records_cached(self, uts):
        c = self._uts_records
        return c[3] if (c is not None and c[0]() is uts and c[1] == uts._version and c[2] == (self.n_entity, self.n_relation)) else None

    def _records_ok(self, uts, caps):        # the records exist, or may be built: the byte cap (a capture that is open raises in _records)
        return self._records_cached(uts) is not None or uts.shape[0] * caps.user_records_words * 4 <= self.USER_RECORDS_MAX_BYTES

    def _records(self, uts):
        """The static per-user records of ``uts``: cached per tensor (identity + version counter, like the one-time id check), else built."""
        rec = self._records_cached(uts)
        if rec is not None:
            return rec
        if self._uts_records is not None and self._uts_records[0]() is None:
            self._uts_records = None     # the tensor the records were built from is gone: free them (up to 8 GiB)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the static per-user records of this user_triplet_set are not built yet: call "
                               "model.prepare(user_triplet_set) before capturing a graph")
        rec = ops.build_user_records(uts, self.p_hop, self.n_relation, self.n_entity)
        self._uts_records = (weakref.ref(uts), uts._version, (self.n_entity, self.n_relation), rec)
        return rec

    # the plan's rules one by one, as bench.py, __graft_entry__.py and the tests read them
    def user_records(self, uts):
        """The static per-user records of a device-resident user_triplet_set, or None when no kernel of this shape / table type reads them."""
        sh, caps, ov, _ = self._route_inputs()
        ok = uts.is_cuda and uts.dtype == torch.int32 and uts.is_contiguous()
        return self._records(uts) if route_plan.wants_records(sh, caps, ov, ok, ok and self._records_ok(uts, caps)) else None

    def _small_static_ok(self):
        sh, caps, _, th = self._route_inputs()
        return route_plan.small_static_ok(sh, caps, th)

    def _small_ok(self, item, memories_h, want_probs):
        """``memories_h`` None = the users feed."""
        sh, caps, ov, th = self._route_inputs()
        return route_plan.small_ok(sh, caps, ov, th, item.shape[0], item.dtype == torch.int64, memories_h is None or memories_h[0].dim() == 2, want_probs)

    def _native_l2_ok(self, item, memories_h, want_probs, cap=True):
        sh, caps, ov, _ = self._route_inputs()
        return route_plan.native_ok(sh, caps, ov, item.shape[0], item.dtype == torch.int64, memories_h is None or memories_h[0].dim() == 2, want_probs, cap)

    def _ka_er_for(self, uts, records):
        sh, caps, ov, _ = self._route_inputs()
        return route_plan.gathered_er(sh, caps, ov, records is not None)

    def _ka_flash_for(self, uts, records, B):
        """(the distinct-users hint: that of the last forward)"""
        sh, caps, ov, th = self._route_inputs()
        return route_plan.flash(sh, caps, ov, th, records is not None, B, uts.shape[0], self._distinct_hint)

    def prepare(self, user_triplet_set=None):
        """Build, eagerly and on the current stream, everything the forward would otherwise build on first use: the
        duplicate-slot encoding of the adjacency (two launches + one host sync), the relation-logit tables of the
        aggregators and -- given a device-resident ``user_triplet_set`` -- its one-time id check and static per-user records
        (an allocation of up to USER_RECORDS_MAX_BYTES + a kernel).  Called by __init__ and set_adjacency for the encoding;
        call it yourself before capturing a forward in a hipGraph or running it on a side stream."""
        if self.fused is not False and self._enc_mode() != "0":      # (forbidden encoding: nothing to build -- 2 launches, a sync, 2 n_entity K words)
            self.encoded_adjacency()
        for agg in self.aggregators:
            if agg.User_orient_rela:
                agg.relation_scores()
        if user_triplet_set is not None:
            self._check_uts(user_triplet_set)
            self.user_records(user_triplet_set)
        return self

    def _build_train(self):
        """model.py:378-414 (loss + Adam): the backward path is a later row of the scope
        table; nothing is built here yet."""
        self.optimizer = None
        self.trainer = None   # created on the first train() call (mvin_amd.training.Trainer)
        self._train_graphs, self._train_seen = {}, None      # captured steps per batch size (train())
        self.train_graph_max_batch = 8192

    def parameters_dict(self):
        """All parameters as numpy arrays under the names of mvin_amd/params.py."""
        L = self.n_mix_hop * self.h_hop
        p = {k: getattr(self, k).float().cpu().numpy() for k in
             ("user_emb_matrix", "entity_emb_matrix", "relation_emb_matrix", "relation_emb_KGE_matrix",
              "user_mlp_matrix", "user_mlp_bias", "h_emb_item_mlp_matrix", "h_emb_item_mlp_bias")}
        for n in range(self.n_mix_hop):
            p[f"enti_transfer_matrix_{n}"] = self.enti_transfer_matrix_list[n].cpu().numpy()
            p[f"enti_transfer_bias_{n}"] = self.enti_transfer_bias_list[n].cpu().numpy()
        for e in range(L + 1):
            p[f"transfer_matrix_{e}"] = self.transfer_matrix_list[e].cpu().numpy()
            p[f"transfer_bias_{e}"] = self.transfer_matrix_bias[e].cpu().numpy()
        for (i, n), agg in self._agg.items():
            tag = f"agg_{i}_{n}_"
            for nm in ("weights", "bias", "urh_weights", "urh_bias"):
                p[tag + nm] = getattr(agg, nm).cpu().numpy()
        return p

    # ------------------------------------------------------------------ stage-wise tables
    _STWS = ("user_emb_matrix", "entity_emb_matrix", "relation_emb_matrix", "relation_emb_KGE_matrix")

    def _emb_path(self):
        if self.path is None or getattr(self.path, "emb", None) is None:
            raise ValueError("args.path.emb is not set")
        return f"{self.path.emb}_sw_para_{self.save_model_name}_parameter.npz"

    def save_pretrain_emb_fuc(self, sess=None, saver=None):
        """model.py:66-67 / train.py:43-51: persist the four ``STWS`` embedding tables."""
        np.savez(self._emb_path(), **{k: getattr(self, k).float().cpu().numpy() for k in self._STWS})

    def restore_pretrain_emb(self):
        """train.py:53-54 counterpart."""
        with np.load(self._emb_path()) as z:
            for k in self._STWS:
                getattr(self, k).copy_(torch.from_numpy(z[k]).to(self.device))   # casts to the table dtype
        self.invalidate()

    def _state_tensors(self):
        """Every parameter tensor by name (the STWS tables, the stacked projections, the MLPs, the aggregators' weights)."""
        p = {k: getattr(self, k) for k in self._STWS + ("user_mlp_matrix", "user_mlp_bias", "_transfer_W", "_transfer_b",
                                                        "h_emb_item_mlp_matrix", "h_emb_item_mlp_bias")}
        for n in range(self.n_mix_hop):
            p[f"enti_transfer_matrix_{n}"] = self.enti_transfer_matrix_list[n]
            p[f"enti_transfer_bias_{n}"] = self.enti_transfer_bias_list[n]
        for (i, n), agg in self._agg.items():
            for nm in ("weights", "bias", "urh_weights", "urh_bias"):
                p[f"agg_{i}_{n}_{nm}"] = getattr(agg, nm)
        return p

    def state(self):
        """Device clones of all parameters, by name: a snapshot ``load_state`` puts back (nothing goes to the host)."""
        return {k: t.clone() for k, t in self._state_tensors().items()}

    def load_state(self, state, names=None):
        """Copy a ``state()`` snapshot (or its ``names`` subset) into the parameters IN PLACE -- a Trainer or captured graph
        that holds their addresses stays valid -- then drop every derived table."""
        mine = self._state_tensors()
        for k in (mine if names is None else names):
            mine[k].copy_(state[k])              # casts to the table dtype
        self.invalidate()

    def load_stws(self, state):
        """The four stage-wise tables of a ``state()`` snapshot (restore_pretrain_emb without the file)."""
        self.load_state(state, self._STWS)

    def invalidate(self):
        """Call after changing parameters in place through raw pointers (the optimizer does):
        drops every derived table (relation logits, hoisted entity tables)."""
        for agg in self.aggregators:
            agg.invalidate()
        self._hoisted = None
        self._generation = getattr(self, "_generation", 0) + 1   # captured hipGraphs of older generations are stale

    # ------------------------------------------------------------------ graph pieces
    def get_neighbors(self, seeds, levels=None):
        """model.py:243-256 on device.  Returns (entities, relations) int32 id lists."""
        L = self.n_mix_hop * self.h_hop if levels is None else levels
        return ops.expand_ids(self.adj_entity, self.adj_relation, seeds, self.n_neighbor, L, self.n_entity)

    def _lookup(self, table, ids32):
        """tf.nn.embedding_lookup of [B] ids -> [B, D]."""
        return ops.linear([table], None, table.shape[-1], ids=[ids32])

    def _key_addressing(self, user32, item32, mem_h, mem_r, mem_t, uts=None, ripple=False):
        """model.py:161-240 -> user_o [B,D].  ``uts``: the ripple sets of pair b are user_triplet_set[user32[b]], indexed inside
        the kernel (mvin_key_addressing_users_fwd) instead of per-pair arrays; ``ripple``: one ops.ripple_attn launch per read."""
        a, D, P = self.args, self.dim, self.p_hop
        B = item32.shape[0]
        nR = self.n_relation
        n_o = P + 1 if a.PS_O_ft else P
        o_cat = torch.empty((B, n_o * D), dtype=torch.float32, device=self.device)
        w_h = self.h_emb_item_mlp_matrix.view(-1) if a.PS_O_ft else None  # first D entries multiply h ([h, user], :171)
        V = None
        if P > 0:
            # V[b,r,:] = E[item_b] . R_KGE[r]   ((R h).v == h.(v R), :214-220)
            V = torch.empty((B, nR, D), dtype=torch.float32, device=self.device)
            ops.linear([self.entity_emb_matrix], self.relation_emb_KGE_matrix, D, ids=[item32], rows=B,
                       out=V, ldo=nR * D, nz=nR, w_zstride=D * D, out_zstride=D)
        if uts is not None:
            ops.key_addressing_users(self.entity_emb_matrix, V, w_h, uts, user32, P, o_cat, n_o * D, nR)
        elif not ripple:
            ops.key_addressing(self.entity_emb_matrix, V, w_h, mem_h, mem_r, mem_t, P, o_cat, n_o * D, nR)
        else:
            slot = 0
            if a.PS_O_ft:  # :162-197, :204-206
                ops.ripple_attn(self.entity_emb_matrix, mem_h[0], None, mem_h[0], None, w_h, 1,
                                o_cat, 0, n_o * D, nR)
                slot = 1
            for hop in range(P):  # :210-230
                ops.ripple_attn(self.entity_emb_matrix, mem_h[hop], mem_r[hop], mem_t[hop], V, None, 0,
                                o_cat, (slot + hop) * D, n_o * D, nR)
        # :232-236
        return ops.linear([o_cat], self.user_mlp_matrix, D, bias=self.user_mlp_bias)

    def _key_addressing_shared(self, item32, mem_h, mem_r, mem_t):
        """model.py:161-240 when EVERY pair of the batch carries the same ripple sets (one user
        scored against many items: the top-K evaluation of util.py:145-181).  ``mem_*``: per hop
        ONE [n_memory] int32 id list.  With the memories fixed the reads turn into dense products
            A[m] = R_KGE[r_m] . E[h_m]         ([Nm, D], once per call)
            logits = E[items] . A^T  ->  softmax over Nm  ->  o = P . E[t]
        on the MFMA linear kernel: ~2 KB of [B, Nm] traffic per pair instead of 2*Nm gathered rows,
        and no [B, nR, D] item projection.  The h-set read (:162-197) does not depend on the item."""
        a, D, P, Nm, nR = self.args, self.dim, self.p_hop, self.n_memory, self.n_relation
        E = self.entity_emb_matrix
        B = item32.shape[0]
        n_o = P + 1 if a.PS_O_ft else P
        o_cat = torch.empty((B, n_o * D), dtype=torch.float32, device=self.device)
        slot0 = 0
        if a.PS_O_ft:
            o1 = torch.empty((1, D), dtype=torch.float32, device=self.device)
            w_h = self.h_emb_item_mlp_matrix.view(-1)
            if ops.key_addressing_supported(Nm, D):
                ops.key_addressing(E, None, w_h, [mem_h[0].view(1, Nm)], [], [], 0, o1, D, nR)
            else:
                ops.ripple_attn(E, mem_h[0].view(1, Nm), None, mem_h[0].view(1, Nm), None, w_h, 1, o1, 0, D, nR)
            o_cat.view(B, n_o, D)[:, 0, :] = o1           # broadcast (plumbing)
            slot0 = 1
        if P > 0:
            Rt = self.relation_emb_KGE_matrix.transpose(1, 2).contiguous()   # W[z] = R[z]^T so that x.W = R.x
            ar = torch.arange(Nm, dtype=torch.int64, device=self.device)
        for hop in range(P):
            Hall = ops.linear([E], Rt, D, ids=[mem_h[hop]], rows=Nm, nz=nR, w_zstride=D * D)     # [nR, Nm, D]
            sel = (mem_r[hop].long() * Nm + ar).to(torch.int32)
            A = ops.linear([Hall.view(nR * Nm, D)], None, D, ids=[sel])                           # [Nm, D]
            logits = ops.linear([E], A.t().contiguous(), Nm, ids=[item32])                        # [B, Nm]
            Pm = ops.row_softmax(logits)
            T = ops.linear([E], None, D, ids=[mem_t[hop]])                                        # [Nm, D] fp32
            ops.linear([Pm], T, D, out=o_cat, out_offset=(slot0 + hop) * D, ldo=n_o * D)
        return ops.linear([o_cat], self.user_mlp_matrix, D, bias=self.user_mlp_bias)

    def _project_levels(self, ents, q, top, need_c=()):
        """model.py:267-283 for levels 0..top-1 (deeper levels are fused into the gather
        kernels).  Returns (ev list, c) where c[e] = q.W_e + b_e ([B, D]) for the levels in
        ``need_c`` and for 1..top-1 (level 0 adds q before the matmul instead)."""
        a, D, K = self.args, self.dim, self.n_neighbor
        B = ents[0].shape[0]
        E = self.entity_emb_matrix
        if not a.User_orient:
            return [ops.linear([E], None, D, ids=[ents[e].view(-1)]).view(B, -1, D) for e in range(top)], {}
        levels = sorted(set(range(1, top)) | set(need_c))
        c = {}
        if levels:
            lo, hi = levels[0], levels[-1] + 1
            cs = ops.linear([q], self._transfer_W[lo:hi], D, bias=self._transfer_b[lo:hi], nz=hi - lo,
                            w_zstride=D * D, bias_zstride=D, out_zstride=B * D)
            cs = cs.view(hi - lo, B, D)
            c = {e: cs[e - lo] for e in range(lo, hi)}
        # level 0: (E[item] + q) . W_0 + b_0 in one launch
        ev = [ops.linear([E, q], self.transfer_matrix_list[0], D, ids=[ents[0].view(-1), None],
                         bias=self.transfer_matrix_bias[0], sum_sources=True).view(B, 1, D)]
        ev += [ops.linear([E], self.transfer_matrix_list[e], D, ids=[ents[e].view(-1)], rowbias=c[e],
                          rows_per_group=K ** e).view(B, -1, D) for e in range(1, top)]
        return ev, c

    def _prof_start(self):
        """``self._profile`` a list (bench.py): HIP events around the launches of the deepest levels."""
        if self._profile is None:
            return None
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        return e

    def _prof_stop(self, e):
        if e is not None:
            e[1].record()
            self._profile.append(e)

    def _apply(self, agg, ev, ents, rels, hop, c, fused_level, want_probs):
        """One aggregator application at one hop (model.py:296-305)."""
        a, D, K = self.args, self.dim, self.n_neighbor
        B = ev[hop].shape[0]
        N = K ** hop
        t = agg.relation_scores() if agg.User_orient_rela else None
        wp = want_probs and agg.User_orient_rela
        if fused_level is not None:
            Wc = self.transfer_matrix_list[fused_level] if a.User_orient else None
            cc = c[fused_level] if a.User_orient else None
            prof = self._prof_start()
            res = ops.gather_attn(self.entity_emb_matrix, self.adj_entity, self.adj_relation,
                                  ents[hop].view(-1), t, ev[hop].view(B * N, D), Wc, cc, agg.weights,
                                  agg.bias, B, N, K, D, want_probs=wp)
            self._prof_stop(prof)
            return res
        return ops.agg(ev[hop].view(B * N, D), ev[hop + 1].view(B * N * K, D), rels[hop].view(-1), t,
                       agg.weights, agg.bias, B, N, K, D, want_probs=wp)

    # ------------------------------------------------------------------ entity-table (hoisted) mode
    def hoist_supported(self):
        a = self.args
        return bool(a.wide_deep and not a.PS_only and self.h_hop >= 2 and self.n_neighbor <= 256)

    def _hoist_key(self):
        a0 = self._agg[(0, 0)]
        ts = (self._transfer_W, self._transfer_b, a0.weights, a0.bias, a0.urh_weights,
              self.relation_emb_matrix, self.adj_entity, self.adj_relation)
        # the entity table: identity + torch version counter, unless its owner writes it behind torch's back
        # (raw-pointer HIP kernels / collectives of dist.ShardedMVIN) and hands out a content token instead
        tok = self._table_token
        ent = (id(self.entity_emb_matrix), self.entity_emb_matrix._version) if tok is None else ("token", tok)
        return (ent,) + tuple((id(t), t._version) for t in ts)

    def hoist_entity_tables(self):
        """Entity-table mode of the two deepest levels (SURVEY.md 7.3-c route 2b; an exact
        re-association of model.py:295-305 + aggregators.py:98-146, not a different model).

        Aggregator (0,0)'s attention weights do not depend on the pair (7.3-a) and everything it
        does below level L-2 before its ReLU is linear in entity rows, so with
            S[e]  = (1/K) sum_k p_k(e) E[adj(e,k)]                 (one gather over ALL entities)
            R1[e] = (E[e].W_{L-1} + S[e].W_L) . A0                  N0[e] = S[e].W_{L-1}
        the per-pair work at a level-(L-2) node x shrinks from K + K^2 row gathers to K + 1:
            neighbors_agg for aggregator (0,0) = N0[x] + c_{L-1}/K        (c/K -> c without the softmax)
            neighbors_agg for aggregator (1,0) = (1/K) sum_k p'_k(x) relu(R1[adj(x,k)] + d)
            d = (c_{L-1} + c_L/K).A0 + a0,  c_e = q.W_e + b_e       (per pair)
        Building costs one pass over n_entity*K rows (~n_entity/K pairs' worth), so it pays as
        soon as a batch holds more level-(L-1) nodes than there are entities; it changes the
        algorithmic bytes per pair and is therefore always reported as its own mode."""
        if not self.hoist_supported():
            raise ValueError("entity-table mode needs wide_deep, h_hop >= 2 and fan-out <= 256")
        D, K = self.dim, self.n_neighbor
        L = self.n_mix_hop * self.h_hop
        E = self.entity_emb_matrix
        a0 = self._agg[(0, 0)]
        h = SimpleNamespace(key=self._hoist_key())
        t0 = a0.relation_scores() if a0.User_orient_rela else None
        S = ops.gather_mix(E, self.adj_entity, self.adj_relation, None, t0, None, self.n_entity, 1, K,
                           self.n_relation)
        if self.args.User_orient:
            W1, W2 = self.transfer_matrix_list[L - 1], self.transfer_matrix_list[L]
            b1, b2 = self.transfer_matrix_bias[L - 1], self.transfer_matrix_bias[L]
            X = ops.linear([E, S], torch.cat([W1, W2]).contiguous(), D)           # E.W1 + S.W2
            h.R1 = ops.linear([X], a0.weights, D)
            h.N0 = ops.linear([S], W1, D)
            # q -> (c1 + c2/K, c1/K) in one launch
            inv = 1.0 / K if a0.User_orient_rela else 1.0   # sum_k w_k / K: softmax weights sum to 1, plain-mean weights to K
            h.Wq = torch.stack([W2, W1]).contiguous()
            h.bq = torch.stack([b2, b1]).contiguous()
            ops.axpby(1.0, W1, inv, h.Wq[0])
            ops.axpby(1.0, b1, inv, h.bq[0])
            ops.axpby(0.0, W1, inv, h.Wq[1])
            ops.axpby(0.0, b1, inv, h.bq[1])
        else:
            h.R1 = ops.linear([E, S], a0.weights, D, sum_sources=True)
            h.N0 = S
        self._hoisted = h
        return h

    def _hoisted_naggs(self, parents, q, B):
        """(neighbors_agg of aggregator (0,0), of aggregator (1,0)) at the level-(L-2) nodes."""
        D, K = self.dim, self.n_neighbor
        h = self._hoisted
        if self.hoist == "step" or h is None or h.key != self._hoist_key():
            h = self.hoist_entity_tables()
        a0, a1 = self._agg[(0, 0)], self._agg[(1, 0)]
        P = parents.numel()
        ppp = P // B
        t1 = a1.relation_scores() if a1.User_orient_rela else None
        if self.args.User_orient:
            cs = ops.linear([q], h.Wq, D, bias=h.bq, nz=2, w_zstride=D * D, bias_zstride=D, out_zstride=B * D)
            cs = cs.view(2, B, D)
            d = ops.linear([cs[0]], a0.weights, D, bias=a0.bias)
            n0 = ops.linear([h.N0], None, D, ids=[parents], rowbias=cs[1], rows_per_group=ppp)
            n1 = ops.gather_mix(h.R1, self.adj_entity, self.adj_relation, parents, t1, d, P, ppp, K,
                                self.n_relation, relu=True)
        else:
            n0 = ops.linear([h.N0], None, D, ids=[parents])
            n1 = ops.gather_mix(h.R1, self.adj_entity, self.adj_relation, parents, t1, a0.bias.view(1, D), P, P, K,
                                self.n_relation, relu=True)
        return n0, n1

    def aggregate_delta_whole(self, item32, q, user_o, want_probs=False):
        """model.py:259-324 -> (item_embeddings [B,D], scores, sigmoid, importance_list).

        Fast path (h_hop >= 2, dim in {16,32,64,128}, fan-out a power of two): the two deepest
        levels run in ONE kernel (mvin_gather_attn_l2_fwd) that returns, per level-(L-2) node,
        the neighbor aggregates consumed by aggregator (0,0) and (1,0) at hop L-2; levels L-1
        and L are never materialised.  Otherwise the per-level kernels are used."""
        D, K, H, M = self.dim, self.n_neighbor, self.h_hop, self.n_mix_hop
        L = M * H
        B = item32.shape[0]
        use_hoist = bool(self.hoist) and not want_probs and self.hoist_supported()
        use_l2 = use_hoist or (self.fused and H >= 2 and ops.gather_attn_l2_supported(D, K))
        top = L - 1 if use_l2 else L          # levels 0..top-1 are materialised
        # depth-2 trees: everything above the fused kernel (level-0 projection, both hop-0 aggregators, the
        # combiner and the score) is ONE launch (mvin_l2_tail_fwd) instead of four
        use_tail = (use_l2 and not use_hoist and L == 2 and M == 1 and self.fused is not False
                    and ops.l2_tail_supported(D))
        if use_tail and item32.dtype == torch.int64:
            # the parents of a depth-2 tree are the items themselves: the fused kernel reads the int64 ids in place
            # (mvin_gather_attn_l2_fwd_i64), no level-0 id list is written
            ents, rels = [item32], []
        else:
            ents, rels = self.get_neighbors(item32, levels=top - 1)
        ev, c = (None, {}) if use_tail else self._project_levels(ents, q, top, need_c=() if use_l2 else (L,))
        nagg = pp = pc = None
        if use_hoist:
            prof = self._prof_start()
            nagg = self._hoisted_naggs(ents[L - 2].view(-1), q, B)
            self._prof_stop(prof)
        elif use_l2:
            a0, a1 = self._agg[(0, 0)], self._agg[(1, 0)]
            uo, E, nE, nR = self.args.User_orient, self.entity_emb_matrix, self.n_entity, self.n_relation
            Wp, bp, Wmix = self.transfer_matrix_list, self.transfer_matrix_bias, self.enti_transfer_matrix_list[0]
            # (this schedule has no gather form of the folded tail; its parents are the level-(L-2) nodes)
            plan = self._l2_plan(B, B * K ** (L - 2), want_probs, use_tail, gather_form=False)
            enc = self.encoded_adjacency() if plan.adjacency == "encoded" else None
            ae, ar = (enc[0], enc[1]) if enc is not None else (self.adj_entity, self.adj_relation)
            parents, ppp = ents[L - 2].view(-1), K ** (L - 2)
            t0, t1 = a0.relation_scores() if a0.User_orient_rela else None, a1.relation_scores() if a1.User_orient_rela else None
            if plan.form == "folded":
                # tables and aggregates from the current parameters, then everything above key addressing in one launch (as mvin_score_l2_fwd)
                fw = self._stream_ws(self._fold_ws, ops._lib.load().mvin_fold_tables_elems(nE, D))
                prof = self._prof_start()
                ops.fold_tables(E, ae, ar, t0, Wp[0], bp[0], Wp[1], bp[1], Wp[2], bp[2], a0.weights, a0.bias, Wmix,
                                self.enti_transfer_bias_list[0], a1.weights, K, nR, out=fw)
                item_emb, scores, sig = ops.score_l2_folded(fw, ae, ar, item32, t0, t1, q, user_o, a1.weights, a1.bias, Wmix, K, D, nR, nE)
                self._prof_stop(prof)
                return item_emb, scores, sig, []
            if plan.form in ("tables", "aggregates"):        # E.W1 | E.W1.A0 | E.W2.A0 from the current parameters, per call
                tabs = ops.project_tables(E, Wp[L - 1], Wp[L], bp[L - 1], bp[L], a0.weights, a0.bias, K, a0.User_orient_rela)
            prof = self._prof_start()
            if plan.form == "aggregates":
                # per-entity aggregates S0 | G of the tables just built: ~cnt rows per parent instead of ~cnt^2
                at = self._stream_ws(self._agg_tables, ops._lib.load().mvin_entity_aggregates_elems(nE, D))
                ops.entity_aggregates(tabs, ae, ar, t0, K, D, nR, nE, out=at)
                n0, n1 = ops.gather_attn_l2_agg(tabs, at, ae, ar, parents, t0, t1, q, B, ppp, K, D, nR, nE)
            elif plan.form == "tables":
                order = ops.order_by_key(ents[0].view(-1)) if plan.item_order else None      # (dropped by the library where no kernel takes it)
                n0, n1 = ops.gather_attn_l2_prj(tabs, ae, ar, parents, t0, t1, q, B, ppp, K, D, nR, nE, encoded=enc is not None, order=order)
            else:
                l2_args = (t0, t1, Wp[L - 1] if uo else None, Wp[L] if uo else None, bp[L - 1] if uo else None, bp[L] if uo else None,
                           q if uo else None, a0.weights, a0.bias, B, ppp, K, D, nR)
                if enc is not None:
                    n0, n1 = ops.gather_attn_l2_enc(E, ae, ar, parents, *l2_args)
                else:
                    n0, n1, pp, pc = ops.gather_attn_l2(E, ae, ar, parents, *l2_args, want_probs=want_probs and a0.User_orient_rela)
            self._prof_stop(prof)
            nagg = (n0, n1)
            if use_tail:
                item_emb, scores, sig = ops.l2_tail(E, item32, q if uo else None, user_o, n0, n1, Wp[0] if uo else None, bp[0] if uo else None,
                                                    a0.weights, a0.bias, a1.weights, a1.bias, Wmix, self.enti_transfer_bias_list[0])
                importance = [pp.view(B, 1, K) if pp is not None else None, pc.view(B, K, K) if pc is not None else None] if want_probs else []
                return item_emb, scores, sig, importance
        importance = []
        out = None
        for n in range(M):
            stages = [ev]
            for i in range(H):
                agg = self._agg[(i, n)]
                nxt, probs = [], []
                for hop in range(L - (H * n + i)):
                    if use_l2 and n == 0 and i == 0 and hop == L - 1:
                        nxt.append(None)  # consumed inside the fused kernel (as nagg[1])
                        probs.append(pc.view(B, K ** (L - 1), K) if pc is not None else None)
                        continue
                    if use_l2 and n == 0 and i <= 1 and hop == L - 2:
                        # aggregators.py:108-116 with neighbors_agg from the fused kernel
                        o = ops.linear([ev[hop].view(-1, D), nagg[i]], agg.weights, D, bias=agg.bias,
                                       relu=True, sum_sources=True).view(B, -1, D)
                        nxt.append(o)
                        probs.append(pp.view(B, K ** (L - 2), K) if (i == 0 and pp is not None) else None)
                        continue
                    fused = L if (not use_l2 and n == 0 and i == 0 and hop == L - 1) else None
                    o, p = self._apply(agg, ev, ents, rels, hop, c, fused, want_probs and i == 0)
                    nxt.append(o)
                    probs.append(p)
                if i == 0:
                    importance = probs
                ev = nxt
                stages.append(ev)
            keep = (M - n - 1) * H + 1
            last = n == M - 1
            new = []
            for e in range(keep):  # :310-315
                res = ops.linear([st[e].view(-1, D) for st in stages], self.enti_transfer_matrix_list[n], D,
                                 bias=self.enti_transfer_bias_list[n], score_u=user_o if last else None)
                if last:
                    out = res
                else:
                    new.append(res.view(B, -1, D))
            ev = new
        item_emb, scores, sig = out
        return item_emb, scores, sig, importance

    def aggregate(self, item32, q, user_o, want_probs=False):
        """model.py:327-376 (wide_deep=False).  The reference revision cannot run this path
        (it treats the aggregator's tuple as a tensor, :366-374); the evident intent --
        element [0] -- is implemented.  Untested by the reference."""
        D, H = self.dim, self.h_hop
        ents, rels = self.get_neighbors(item32, levels=H - 1)
        ev, c = self._project_levels(ents, q, H, need_c=(H,))
        for i in range(H):
            agg = self._agg[(i, 0)]
            nxt = []
            for hop in range(H - i):
                fused = H if (i == 0 and hop == H - 1) else None
                o, _ = self._apply(agg, ev, ents, rels, hop, c, fused, False)
                nxt.append(o)
            ev = nxt
        item_emb, scores, sig = ops.linear([ev[0].view(-1, D)], None, D, score_u=user_o)
        return item_emb, scores, sig, []

    # ------------------------------------------------------------------ forward
    def forward_users(self, user_indices, item_indices, user_triplet_set, want_probs=False, distinct_users=None):
        """The same pass when the caller holds ``user_triplet_set`` on the device ([n_user, max(1,P), 3, n_memory]
        int32, data_loader_user_set.py:392-441) instead of per-pair ripple-set arrays: the feed assembly of
        train.py:117-120 (memories_x[i] = user_triplet_set[user][i][x]) happens inside the key-addressing kernel,
        which groups the batch's pairs by user and reads each user's rows once (``_key_addressing_grouped``).
        ``distinct_users``: how many different users the caller expects in THIS batch when it knows better than
        "any of n_user" (a rank that scores the pairs of 1/W of the users; a top-K evaluation over 250 users): the
        static pairs-per-user rule that picks the grouped form uses it instead of n_user."""
        return self.forward_device(user_indices, item_indices, None, None, None, want_probs=want_probs,
                                   uts=user_triplet_set, distinct_users=distinct_users)

    # ------------------------------------------------------------------ native whole-pass schedule
    def _score_args_static(self, depth=None):
        """The static half of ScoreL2Args -- adjacency, KGE, MLPs, projections, aggregators, mix, shape words -- and the tensors whose
        addresses it holds (kept alive with the block; rebinding a parameter attribute needs invalidate(), as for the cached relation
        logits).  ``depth``: the single-launch pass takes trees of depth 1 or 2, passes the depth and has W_e / b_e for e <= depth only
        (a one-hop tree has aggregator (0,0) only); None: mvin_score_l2_fwd, depth-2 trees."""
        from . import _lib
        a, L = self.args, 2 if depth is None else depth
        ptr = lambda t: t.data_ptr() if t is not None else None
        a0, a1 = self._agg[(0, 0)], self._agg.get((1, 0))
        s = _lib.ScoreL2Args()
        s.adj_entity, s.adj_relation = ptr(self.adj_entity), ptr(self.adj_relation)
        s.relation_kge = ptr(self.relation_emb_KGE_matrix)
        s.h_set_w = ptr(self.h_emb_item_mlp_matrix) if a.PS_O_ft else None
        s.user_mlp_W, s.user_mlp_b = ptr(self.user_mlp_matrix), ptr(self.user_mlp_bias)
        for e in range(3):
            setattr(s, f"W{e}", ptr(self.transfer_matrix_list[e]) if (a.User_orient and e <= L) else None)
            setattr(s, f"b{e}", ptr(self.transfer_matrix_bias[e]) if (a.User_orient and e <= L) else None)
        s.A0, s.a0 = ptr(a0.weights), ptr(a0.bias)
        s.A1, s.a1 = (ptr(a1.weights), ptr(a1.bias)) if a1 is not None else (None, None)
        s.Wmix, s.bmix = ptr(self.enti_transfer_matrix_list[0]), ptr(self.enti_transfer_bias_list[0])
        s.D, s.K, s.P, s.Nm = self.dim, self.n_neighbor, self.p_hop, self.n_memory
        s.n_entity, s.n_relation = self.n_entity, self.n_relation
        s.depth = depth or 0
        keep = (self.adj_entity, self.adj_relation, self.relation_emb_KGE_matrix, self.h_emb_item_mlp_matrix,
                self.user_mlp_matrix, self.user_mlp_bias, list(self.transfer_matrix_list), list(self.transfer_matrix_bias),
                a0.weights, a0.bias, a1.weights if a1 is not None else None, a1.bias if a1 is not None else None,
                self.enti_transfer_matrix_list[0], self.enti_transfer_bias_list[0])
        return s, keep

    def _score_small_native(self, item, mem_h, mem_r, mem_t, uts=None, users=None):
        """model.py:125-159 as ONE kernel launch (mvin_score_small_fwd).  The argument block is built once per parameter
        generation; per call only the table / logit-table / feed / output pointers are refreshed and ONE output buffer is
        allocated (the four result tensors are views made when somebody reads them: the host side of this path is as long
        as its kernel)."""
        from . import _lib
        import ctypes as C
        D, P, B = self.dim, self.p_hop, item.shape[0]
        a0, a1 = self._agg[(0, 0)], self._agg.get((1, 0))          # a one-hop tree (h_hop = 1) has aggregator (0,0) only
        t0 = a0.relation_scores() if a0.User_orient_rela else None
        t1 = a1.relation_scores() if (a1 is not None and a1.User_orient_rela) else None
        st = self._small_state
        if st is None or st["key"] != self._generation or st["dedup"] != self.dedup:
            s, keep = self._score_args_static(depth=self.h_hop)
            s.table_bf16 = 0
            # the duplicate-slot encoding whenever the adjacency has one (distinct rows only; a row without repeats costs the
            # same either way) unless the plain adjacency is forced (MVIN.dedup = False / MVIN_L2_ENC=0)
            enc = self.encoded_adjacency() if self._enc_mode() != "0" else None
            s.enc_entity, s.enc_relation = (enc[0].data_ptr(), enc[1].data_ptr()) if enc is not None else (None, None)
            keep += (enc,)
            st = self._small_state = {"key": self._generation, "args": s, "ref": C.byref(s), "keep": keep, "arr": (C.c_void_p * P),
                                      "dedup": self.dedup, "fn": _lib.load().mvin_score_small_fwd, "live": None}
        s = st["args"]
        E = self.entity_emb_matrix
        s.entity_emb = E.data_ptr()
        s.t0 = t0.data_ptr() if t0 is not None else None
        s.t1 = t1.data_ptr() if t1 is not None else None
        out = torch.empty((2 * B * D + 2 * B,), dtype=torch.float32, device=self.device)      # one allocation for the four outputs
        s.items = item.data_ptr()
        if uts is not None:
            s.uts, s.users, s.n_user = uts.data_ptr(), users.data_ptr(), uts.shape[0]
            s.mem_h = s.mem_r = s.mem_t = None
        else:
            arr = st["arr"]
            hold = (arr(*[t.data_ptr() for t in mem_h[:P]]), arr(*[t.data_ptr() for t in mem_r[:P]]),
                    arr(*[t.data_ptr() for t in mem_t[:P]]))
            st["live"] = hold                 # (read by the call below only; kept until the next call replaces it)
            s.uts = s.users = None
            s.mem_h, s.mem_r, s.mem_t = C.addressof(hold[0]), C.addressof(hold[1]), C.addressof(hold[2])
        base = out.data_ptr()
        s.user_o, s.item_emb, s.scores, s.sig = base, base + 4 * B * D, base + 8 * B * D, base + 8 * B * D + 4 * B
        s.B = B
        rc = st["fn"](st["ref"], self.small_group, torch.cuda.current_stream().cuda_stream)
        if rc:
            _lib.check(rc, "mvin_score_small_fwd")
        return _SmallOut(out, B, D)

    def _score_l2_native(self, item, mem_h, mem_r, mem_t, uts=None, users=None, grouped=False, ka="per_pair", records=False):
        """model.py:125-159 through mvin_score_l2_fwd.  The argument block (every weight pointer) is built once and
        kept until a parameter tensor is replaced; per call only the batch pointers change.  ``grouped`` / ``ka`` / ``records``: the
        route's decision (pairs grouped by user, its key-addressing form, the static records go along)."""
        from . import _lib
        import ctypes as C
        a, D, P, B = self.args, self.dim, self.p_hop, item.shape[0]
        a0, a1 = self._agg[(0, 0)], self._agg[(1, 0)]
        t0, t1 = a0.relation_scores() if a0.User_orient_rela else None, a1.relation_scores() if a1.User_orient_rela else None
        # The block is rebuilt when a parameter tensor may have been REPLACED (generation); what legitimately changes
        # from call to call -- the entity table (ShardedMVIN alternates two working tables), the relation-logit tables
        # (rebuilt after every optimizer step) and the batch -- is refreshed per call, and the workspaces live outside
        # the block, per (batch size, stream): no allocation churn on the small-batch path this call exists for, and
        # two streams scoring the same batch size never share V / o_cat / nagg.
        ptr = lambda t: t.data_ptr() if t is not None else None
        st = self._native_l2_state
        if st is None or st["key"] != self._generation:
            s, keep = self._score_args_static()
            st = self._native_l2_state = {"key": self._generation, "args": s, "keep": keep, "arr": (C.c_void_p * P)}
        s = st["args"]
        s.entity_emb, s.t0, s.t1 = ptr(self.entity_emb_matrix), ptr(t0), ptr(t1)
        s.table_bf16 = 1 if self.entity_emb_matrix.dtype == torch.bfloat16 else 0
        # (depth-2 trees: the parents are the pairs; this call has the one-launch tail and the gather form of the folded tail)
        plan = self._l2_plan(B, B)
        form = plan.form
        enc = self.encoded_adjacency() if plan.adjacency == "encoded" else None
        s.enc_entity, s.enc_relation = (ptr(enc[0]), ptr(enc[1])) if enc is not None else (None, None)
        rec = self._records(uts) if records else None
        s.user_records = ptr(rec)
        st["live"] = (self.entity_emb_matrix, t0, t1, enc, rec)
        s.ka_er = s.ka_flash = None
        stream = torch.cuda.current_stream()
        cs, lib = stream.cuda_stream, _lib.load()
        if ka == "flash":            # its tables are rebuilt by every call
            s.ka_flash = self._stream_ws(self._ka_flash_ws, self._route_shape_caps()[1].flash_tables_elems, stream=cs).data_ptr()
        elif ka == "gathered_er":    # gathered U rows: the table is rebuilt by every call
            s.ka_er = self._stream_ws(self._ka_er_ws, lib.mvin_project_relations_elems(self.n_entity, self.n_relation, D), stream=cs).data_ptr()
        n_o = P + (1 if a.PS_O_ft else 0)
        # projected tables: E.W1 | E.W1.A0 | E.W2.A0 is rebuilt by every call from the current parameters (~n_entity rows of work against
        # ~B K / 4); the aggregates are built from those tables, the folded forms hold their own tables in their own workspace
        s.prj_tables = s.agg_tables = s.fold_ws = None
        if form in ("tables", "aggregates"):
            s.prj_tables = self._stream_ws(self._prj_tables, lib.mvin_project_tables_elems(self.n_entity, D), stream=cs).data_ptr()
        if form == "aggregates":
            s.agg_tables = self._stream_ws(self._agg_tables, lib.mvin_entity_aggregates_elems(self.n_entity, D), stream=cs).data_ptr()
        elif form in ("folded", "folded_gather"):
            s.fold_ws = self._stream_ws(self._fold_ws, lib.mvin_fold_tables_elems(self.n_entity, D), stream=cs).data_ptr()
        s.fold_gather = 1 if form == "folded_gather" else 0
        wkey = (B, n_o, cs, bool(grouped), uts.shape[0] if grouped else 0)
        ws = self._native_l2_ws.get(wkey)
        if ws is None:        # reused across calls of the same batch size ON THE SAME STREAM (which orders the reuse)
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
            # grouped key addressing needs no [B, nR, D] item projection; its sort workspace instead
            gws = torch.empty(ops.score_group_ws_elems(uts.shape[0], B), dtype=torch.int32, device=self.device) if grouped else None
            ows = None                    # (the item-order workspace: allocated when first wanted, below)
            ws = self._native_l2_ws[wkey] = (None if grouped else f(B, self.n_relation, D), f(B, n_o * D),
                                             torch.empty(B, dtype=torch.int32, device=self.device), f(B, D), f(B, D), gws, ows)
            if len(self._native_l2_ws) > 8:
                self._native_l2_ws.pop(next(iter(self._native_l2_ws)))
        user_o, item_emb = torch.empty((B, D), dtype=torch.float32, device=self.device), torch.empty((B, D), dtype=torch.float32, device=self.device)
        scores, sig = torch.empty((B,), dtype=torch.float32, device=self.device), torch.empty((B,), dtype=torch.float32, device=self.device)
        s.items = item.data_ptr()
        if uts is not None:       # users feed: the kernel reads the lists of users[b] out of user_triplet_set
            s.uts, s.users, s.n_user = uts.data_ptr(), users.data_ptr(), uts.shape[0]
            s.mem_h = s.mem_r = s.mem_t = None
        else:
            ph, pr, pt = (st["arr"](*[t.data_ptr() for t in lst[:P]]) for lst in (mem_h, mem_r, mem_t))
            s.uts = s.users = None
            s.mem_h, s.mem_r, s.mem_t = C.addressof(ph), C.addressof(pr), C.addressof(pt)
        s.V, s.o_cat, s.parents, s.nagg0, s.nagg1, s.group_ws = (w.data_ptr() if w is not None else None for w in ws[:6])
        s.item_order_ws = None
        if plan.item_order:
            if ws[6] is None:
                ws = self._native_l2_ws[wkey] = ws[:6] + (torch.empty(lib.mvin_order_by_key_ws_elems(B) + B, dtype=torch.int32, device=self.device),)
            s.item_order_ws = ws[6].data_ptr()
        s.user_o, s.item_emb, s.scores, s.sig = user_o.data_ptr(), item_emb.data_ptr(), scores.data_ptr(), sig.data_ptr()
        s.B = B
        _lib.check(lib.mvin_score_l2_fwd(C.byref(s), C.c_void_p(cs)), "mvin_score_l2_fwd")
        return SimpleNamespace(scores=scores, scores_normalized=sig, user_o=user_o, item_embeddings=item_emb,
                               importance_list=[])

    def _key_addressing_grouped(self, user, item, uts, form, records):
        """model.py:161-240 with the pairs grouped by user (mvin_key_addressing_grouped_fwd) -> user_o [B,D].  ``form``: the route's
        key-addressing form (route_plan.GROUPED_FORMS); ``records``: the call wants the static per-user records."""
        a, D, P = self.args, self.dim, self.p_hop
        n_o = P + 1 if a.PS_O_ft else P
        o_cat = torch.empty((item.shape[0], n_o * D), dtype=torch.float32, device=self.device)
        w_h = self.h_emb_item_mlp_matrix.view(-1) if a.PS_O_ft else None
        groups = ops.group_pairs_by_user(user, n_user=uts.shape[0])
        rec = self._records(uts) if records else None
        if form == "flash":
            kp = getattr(self, "_ka_profile", None)      # bench.py: HIP events around the table build and the kernel
            if kp is not None:
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                evs[0].record()
            tabs = ops.key_addressing_flash_prepare(self.entity_emb_matrix, self.relation_emb_KGE_matrix, w_h, self.user_mlp_matrix, P,
                                                    out=self._stream_ws(self._ka_flash_ws, self._route_shape_caps()[1].flash_tables_elems))
            if kp is not None:
                evs[1].record()
            uo = ops.key_addressing_flash(self.entity_emb_matrix, tabs, rec, groups, item, P, self.n_memory, self.n_relation,
                                          w_h is not None, self.user_mlp_bias, uts.shape[0])
            if kp is not None:
                evs[2].record()
                kp.append(evs)
            return uo
        er = ops.project_relations(self.entity_emb_matrix, self.relation_emb_KGE_matrix, w_h) if form == "gathered_er" else None
        ops.key_addressing_grouped(self.entity_emb_matrix, self.relation_emb_KGE_matrix, w_h, uts, groups, item, P,
                                   o_cat, n_o * D, self.n_relation, records=rec if form in route_plan.RECORD_FORMS else None, er=er)
        return ops.linear([o_cat], self.user_mlp_matrix, D, bias=self.user_mlp_bias)

    def forward_device(self, user_indices, item_indices, memories_h, memories_r, memories_t,
                       want_probs=False, uts=None, distinct_users=None):
        """model.py:125-159 on device-resident inputs (int64/int32 ids [B]; int32 ripple sets
        [B, n_memory] per hop).  Returns a namespace of device tensors.
        Shared-user form: ripple sets given as ONE [n_memory] list per hop (and ``user_indices`` a
        single id or [B]) score one user against ``item_indices`` -- see ``_key_addressing_shared``.
        ``uts`` (instead of the memories): see ``forward_users``.  Which schedule, feed and key-addressing form the call
        takes: ``_route`` (mvin_amd/route_plan.py)."""
        a = self.args
        if not item_indices.is_cuda:
            raise RuntimeError("forward_device needs device-resident inputs (no CPU path)")
        self._distinct_hint = distinct_users
        item32 = item_indices.contiguous()   # int64 (reference dtype) or int32: kernels take both
        user32 = user_indices.contiguous()
        if uts is not None:
            self._check_uts(uts)
            memories_h = memories_r = memories_t = None
        if self.validate_device_ids:
            self._check_device_ids(item32, self.n_entity, "item_indices")
            self._check_device_ids(user32, uts.shape[0] if uts is not None else self.n_user, "user_indices")
            for lst, lim, what in ((memories_h, self.n_entity, "memories_h"), (memories_r, self.n_relation, "memories_r"),
                                   (memories_t, self.n_entity, "memories_t")):
                for m_ in (lst or ()):
                    self._check_device_ids(m_, lim, what)
        route = self._route(user32, item32, memories_h, memories_r, memories_t, uts, want_probs, distinct_users)
        schedule, feed, ka = route.schedule, route.feed, route.key_addressing
        B = item32.shape[0]
        if route.broadcast_user:
            user32 = user32.reshape(1).expand(B).contiguous()
        if schedule == "small" and feed != "assembled":            # ONE launch
            return (self._score_small_native(item32, None, None, None, uts=uts, users=user32) if feed == "users"
                    else self._score_small_native(item32, memories_h, memories_r, memories_t))
        if feed == "assembled":              # any other wiring: assemble the per-pair feeds on the device
            sel = uts[user32.long()]
            memories_h, memories_r, memories_t = ([sel[:, i, x].contiguous() for i in range(sel.shape[1])] for x in range(3))
        elif feed == "pairs" and memories_h is not None and memories_h[0].dim() == 1:
            # one shared list outside the dense form (the [B, Nm] logits go through mvin_linear_fwd): replicate the sets
            rep = lambda lst: [m_.reshape(1, -1).expand(B, -1).contiguous() for m_ in lst]
            memories_h, memories_r, memories_t = rep(memories_h), rep(memories_r), rep(memories_t)
        if schedule == "small":
            return self._score_small_native(item32, memories_h, memories_r, memories_t)
        if schedule == "native":
            # one native call; key addressing indexes user_triplet_set by users[b] itself, or -- grouped -- sorts the batch by user on
            # the device first; else it reads the per-pair lists
            if feed == "users":
                return self._score_l2_native(item32, None, None, None, uts=uts, users=user32, grouped=ka in route_plan.GROUPED_FORMS,
                                             ka=ka, records=route.records)
            return self._score_l2_native(item32, memories_h, memories_r, memories_t)
        if ka == "none":
            ps = None
        elif ka in route_plan.GROUPED_FORMS:
            ps = self._key_addressing_grouped(user32, item32, uts, ka, route.records)
        elif ka == "users_feed":
            # key addressing reads the lists of users[b] out of user_triplet_set itself -- it was a torch gather + three copies per
            # step to assemble them
            ps = self._key_addressing(user32, item32, None, None, None, uts=uts)
        elif ka == "shared":
            ps = self._key_addressing_shared(item32, [m_.contiguous() for m_ in memories_h],
                                             [m_.contiguous() for m_ in memories_r],
                                             [m_.contiguous() for m_ in memories_t])
        else:
            ps = self._key_addressing(user32, item32, memories_h, memories_r, memories_t, ripple=ka == "ripple")
        importance = []
        if a.PS_only:  # :142-144
            user_o = ps
            item_emb, scores, sig = ops.linear([self.entity_emb_matrix], None, self.dim, ids=[item32],
                                               score_u=user_o)
        else:
            user_o = self._lookup(self.user_emb_matrix, user32) if a.HO_only else ps
            if a.User_orient_kg_eh:
                q = ps
            else:
                q = user_o if a.HO_only else self._lookup(self.user_emb_matrix, user32)
            item_emb, scores, sig, importance = self.agg_fun(item32, q, user_o, want_probs)
        return SimpleNamespace(scores=scores, scores_normalized=sig, user_o=user_o,
                               item_embeddings=item_emb, importance_list=importance)

    # ------------------------------------------------------------------ feed handling
    def _check_uts(self, uts):
        """A device-resident user_triplet_set is validated ONCE per tensor (identity + torch version): the grouped /
        users-feed kernels index the entity table, the relation matrices and LDS with its entries."""
        # identity of the tensor OBJECT (a weak reference: a freed tensor's address is reused by the caching allocator) and its
        # torch version counter; the kernels clamp every id they index memory with, so this check is about raising the
        # reference's IndexError, not about memory safety
        ok = self._uts_ok
        if ok is not None and ok[0]() is uts and ok[1] == uts._version:
            return
        if uts.dim() != 4 or uts.shape[2] != 3 or uts.shape[1] != max(1, self.p_hop) or uts.shape[3] != self.n_memory:
            raise ValueError(f"user_triplet_set must be [n_user, {max(1, self.p_hop)}, 3, {self.n_memory}], "
                             f"got {tuple(uts.shape)}")
        P = self.p_hop
        bad = (uts[:, :, 0] < 0).any() | (uts[:, :, 0] >= self.n_entity).any()
        if P > 0:
            r, t = uts[:, :P, 1], uts[:, :P, 2]
            bad = bad | (r < 0).any() | (r >= self.n_relation).any() | (t < 0).any() | (t >= self.n_entity).any()
        if bool(bad.item()):
            raise IndexError("user_triplet_set: id out of range (heads / tails in [0, n_entity), relations in [0, n_relation))")
        self._uts_ok = (weakref.ref(uts), uts._version)

    def _check_device_ids(self, t, limit, what):
        if t is not None and t.numel() and bool(((t < 0) | (t >= limit)).any().item()):
            raise IndexError(f"{what}: id out of range [0, {limit})")

    def _to_device_ids(self, v, dtype, limit, what):
        if isinstance(v, torch.Tensor):
            t = v
            if not t.is_cuda:
                t = t.to(self.device)
            return t.to(dtype).contiguous()
        arr = np.asarray(v)
        if arr.size and (arr.min() < 0 or arr.max() >= limit):
            # the reference's CPU tf.gather raises InvalidArgument on out-of-range ids
            raise IndexError(f"{what}: id out of range [0, {limit})")
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self.device).to(dtype).contiguous()

    def _feed(self, feed_dict):
        n_lists = max(1, self.p_hop)
        user = self._to_device_ids(feed_dict[self.user_indices], torch.int64, self.n_user, "user_indices")
        item = self._to_device_ids(feed_dict[self.item_indices], torch.int64, self.n_entity, "item_indices")
        mh = [self._to_device_ids(feed_dict[self.memories_h[i]], torch.int32, self.n_entity, "memories_h")
              for i in range(n_lists)]
        mr = [self._to_device_ids(feed_dict[self.memories_r[i]], torch.int32, self.n_relation, "memories_r")
              for i in range(n_lists)]
        mt = [self._to_device_ids(feed_dict[self.memories_t[i]], torch.int32, self.n_entity, "memories_t")
              for i in range(n_lists)]
        return user, item, mh, mr, mt

    # ------------------------------------------------------------------ run wrappers
    def train(self, sess, feed_dict):
        """model.py:416-417: one optimisation step (forward, loss of :378-412, backward, Adam of :414)
        on the GPU -> (None, loss).  The optimizer state lives in ``self.trainer``."""
        if self.trainer is None:
            from .training import Trainer
            self.trainer = Trainer(self)
        user, item, mh, mr, mt = self._feed(feed_dict)
        labels = torch.as_tensor(np.asarray(feed_dict[self.labels], dtype=np.float32)).to(self.device)
        # The reference trains at ONE batch size (train.py:56-64: `start += args.batch_size`, one sess.run per batch) and a step
        # at 512 / 1 024 pairs is ~60 short launches: from the second step of a batch size on, the step is one hipGraph replay
        # (training.GraphedTrainer: 0.68 vs 1.00 ms at 512 pairs).  MVIN_TRAIN_GRAPH=0, a multi-rank trainer or a batch above
        # train_graph_max_batch keep the eager launches; the first step of a size runs eagerly (it is the capture's warm-up).
        B = int(item.shape[0])
        if (os.environ.get("MVIN_TRAIN_GRAPH", "1") != "0" and self.trainer.world == 1 and B <= self.train_graph_max_batch):
            from .training import GraphedTrainer
            g = self._train_graphs.get(B)
            if g is False:
                g = None
            elif g is not None and (g._storage_key() != g._captured
                                    or g.head != self.trainer.head_key()
                                    or g.guard != self.trainer.guard_key()):
                g = None                   # adjacency / a parameter tensor replaced, another objective or guard: capture again
            if g is None and self._train_seen == B and self._train_graphs.get(B) is not False:
                try:
                    g = self._train_graphs[B] = GraphedTrainer(self.trainer, B, ids_dtype=item.dtype, warmup=0)
                except RuntimeError:
                    # a step that cannot be captured (a kernel or allocation that refuses to run under capture) still runs
                    # eagerly: remember the failure for this batch size and fall through (train_epoch_device does the same)
                    g, self._train_graphs[B] = None, False
                if len(self._train_graphs) > 4:
                    self._train_graphs.pop(next(iter(self._train_graphs)))
            self._train_seen = B
            if g:
                return None, float(g.step(user, item, labels, mh, mr, mt).item())
        return None, self.trainer.step(user, item, labels, mh, mr, mt)

    def get_scores(self, sess, feed_dict):
        """model.py:443-444."""
        user, item, mh, mr, mt = self._feed(feed_dict)
        out = self.forward_device(user, item, mh, mr, mt)
        return item.cpu().numpy(), out.scores_normalized.cpu().numpy()

    def eval(self, sess, feed_dict):
        """model.py:419-426."""
        from sklearn.metrics import f1_score, roc_auc_score
        user, item, mh, mr, mt = self._feed(feed_dict)
        labels = np.asarray(feed_dict[self.labels], dtype=np.float32)
        scores = self.forward_device(user, item, mh, mr, mt).scores_normalized.cpu().numpy()
        auc = roc_auc_score(y_true=labels, y_score=scores)
        scores[scores >= 0.5] = 1
        scores[scores < 0.5] = 0
        f1 = f1_score(y_true=labels, y_pred=scores)
        acc = np.mean(np.equal(scores, labels))
        return auc, acc, f1

    def eval_case_study(self, sess, feed_dict):
        """model.py:428-441: ids of every level plus the attention weights of the i=0 pass."""
        user, item, mh, mr, mt = self._feed(feed_dict)
        out = self.forward_device(user, item, mh, mr, mt, want_probs=True)
        L = self.n_mix_hop * self.h_hop
        ents, rels = self.get_neighbors(item.to(torch.int32), levels=L)
        imp = out.importance_list
        imp0 = imp[0].cpu().numpy() if imp and imp[0] is not None else None
        imp1 = imp[1].cpu().numpy() if len(imp) > 1 and imp[1] is not None else 0
        return (user.cpu().numpy(), np.asarray(feed_dict[self.labels], dtype=np.float32), item.cpu().numpy(),   # fetched placeholder: float32 (model.py:52)
                [e.cpu().numpy().astype(np.int64) for e in ents],
                [r.cpu().numpy().astype(np.int64) for r in rels], imp0, imp1)
