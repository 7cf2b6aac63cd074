"""Torch-tensor front end of the C ABI (include/mvin_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; all arithmetic of the
path runs in libmvin_hip.so.  Every op requires CUDA(ROCm) tensors and raises otherwise --
there is no CPU / eager fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

F32 = torch.float32
I32 = torch.int32
BF16 = torch.bfloat16


def _chk_table(t, name):
    """Entity-style table: fp32 or bf16 (bf16 rows are widened to fp32 inside the kernels)."""
    if t is None:
        return 0
    _chk(t, BF16 if t.dtype == BF16 else F32, name)
    return 1 if t.dtype == BF16 else 0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def _p(t, offset_elems=0):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def ent_level_offsets(B, K, levels):
    """Element offsets of entity levels 0..levels and relation levels 0..levels-1 in the
    flat buffers written by mvin_expand_ids (see include/mvin_hip.h)."""
    ent, rel, off_e, off_r, n = [], [], 0, 0, B
    for e in range(levels + 1):
        ent.append((off_e, n))
        off_e += n
        if e < levels:
            n *= K
            rel.append((off_r, n))
            off_r += n
    return ent, rel


def expand_ids(adj_entity, adj_relation, items, K, levels, n_entity):
    """MVIN.get_neighbors (model.py:243-256).  Returns (entities, relations): lists of int32
    tensors [B, K^e] (e = 0..levels) and [B, K^(e+1)] (e = 0..levels-1), views of two flat
    buffers."""
    lib = _lib.load()
    _chk(adj_entity, I32, "adj_entity")
    _chk(adj_relation, I32, "adj_relation")
    if items.dtype == torch.int64:
        i64, i32 = _chk(items, torch.int64, "items"), None
    else:
        i64, i32 = None, _chk(items, I32, "items")
    B = items.shape[0]
    ent_flat = torch.empty(lib.mvin_ent_elems(B, K, levels), dtype=I32, device=items.device)
    rel_flat = torch.empty(max(1, lib.mvin_rel_elems(B, K, levels)), dtype=I32, device=items.device)
    _lib.check(lib.mvin_expand_ids(_p(adj_entity), _p(adj_relation), _p(i64), _p(i32), B, K, levels,
                                   n_entity, _p(ent_flat), _p(rel_flat), _stream()), "mvin_expand_ids")
    eo, ro = ent_level_offsets(B, K, levels)
    ents = [ent_flat[o:o + n].view(B, -1) for o, n in eo]
    rels = [rel_flat[o:o + n].view(B, -1) for o, n in ro]
    return ents, rels


def rel_score(relation_emb, urh_weights):
    """t[r] = relation_emb[r] . urh_weights[D:2D]  (aggregators.py:130-133, k-dependent term)."""
    lib = _lib.load()
    _chk(relation_emb, F32, "relation_emb")
    _chk(urh_weights, F32, "urh_weights")
    nR, D = relation_emb.shape
    t = torch.empty(nR, dtype=F32, device=relation_emb.device)
    _lib.check(lib.mvin_rel_score(_p(relation_emb), _p(urh_weights), nR, D, _p(t), _stream()),
               "mvin_rel_score")
    return t


def linear(srcs, W, Dout, *, ids=None, bias=None, rowbias=None, rows_per_group=1, relu=False,
           rows=None, out=None, out_offset=0, ldo=None, nz=1, w_zstride=0, bias_zstride=0,
           out_zstride=0, score_u=None, sum_sources=False):
    """mvin_linear_fwd: out[z][r] = act(concat_s X_s[r] . W[z] + bias[z] + rowbias[r // rpg]).
    ``srcs``: list of [*, Dsrc] fp32 tensors; ``ids``: matching list of int32 row-id tensors
    or None.  Returns out, or (out, score, sigmoid) when ``score_u`` is given."""
    lib = _lib.load()
    a = _lib.LinearArgs()
    nsrc = len(srcs)
    ids = ids or [None] * nsrc
    ids64 = None
    Dsrc = srcs[0].shape[-1]
    src_bf16 = 0
    for s in range(nsrc):
        src_bf16 |= _chk_table(srcs[s], f"src[{s}]") << s
        if srcs[s].shape[-1] != Dsrc:
            raise ValueError("all sources must share the row width")
        a.src[s] = srcs[s].data_ptr()
        if ids[s] is not None:
            if ids64 is None:
                ids64 = ids[s].dtype == torch.int64
            _chk(ids[s], torch.int64 if ids64 else I32, f"ids[{s}]")
            a.ids[s] = ids[s].data_ptr()
    if rows is None:
        first = next((i for i in ids if i is not None), None)
        rows = first.numel() if first is not None else srcs[0].numel() // Dsrc
    dev = srcs[0].device
    if out is None:
        ldo = ldo or Dout
        out = torch.empty((nz, rows, Dout) if nz > 1 else (rows, Dout), dtype=F32, device=dev)
        if nz > 1 and out_zstride == 0:
            out_zstride = rows * Dout
    else:
        _chk(out, F32, "out")
        ldo = ldo or Dout
    a.nsrc, a.Dsrc, a.Dout, a.rows = nsrc, Dsrc, Dout, rows
    a.W = _chk(W, F32, "W").data_ptr() if W is not None else None
    a.bias = _chk(bias, F32, "bias").data_ptr() if bias is not None else None
    a.rowbias = _chk(rowbias, F32, "rowbias").data_ptr() if rowbias is not None else None
    a.rows_per_group = rows_per_group
    a.relu = 1 if relu else 0
    a.ids64 = 1 if ids64 else 0
    a.src_bf16 = src_bf16
    gathered = [srcs[s].numel() // Dsrc for s in range(nsrc) if ids[s] is not None]
    if len(set(gathered)) > 1:
        # mvin_linear_args carries ONE src_rows: ids valid for the larger table would be clamped to the smaller one's last row
        raise ValueError(f"gathered sources of one mvin_linear_fwd call must have the same row count, got {gathered}")
    a.src_rows = gathered[0] if gathered else 0           # ids are clamped into the gathered table
    a.sum_sources = 1 if sum_sources else 0
    a.out = out.data_ptr() + out_offset * 4
    a.ldo = ldo
    a.nz, a.w_zstride, a.bias_zstride, a.out_zstride = nz, w_zstride, bias_zstride, out_zstride
    score = sig = None
    if score_u is not None:
        _chk(score_u, F32, "score_u")
        score = torch.empty(rows, dtype=F32, device=dev)
        sig = torch.empty(rows, dtype=F32, device=dev)
        a.score_u, a.score_out, a.sigmoid_out = score_u.data_ptr(), score.data_ptr(), sig.data_ptr()
    _lib.check(lib.mvin_linear_fwd(C.byref(a), _stream()), "mvin_linear_fwd")
    return (out, score, sig) if score_u is not None else out


def score_small_supported(D, K, P, Nm, nR):
    """mvin_score_small_supported: the whole depth-2 pass as one launch exists for this shape."""
    return bool(_lib.load().mvin_score_small_supported(int(D), int(K), int(P), int(Nm), int(nR)))


def score_small(entity_emb, adj_entity, adj_relation, relation_kge, h_set_w, user_mlp_W, user_mlp_b, t0, t1, W0, b0, W1, b1, W2, b2,
                A0, a0, A1, a1, Wmix, bmix, items, *, mem_h=None, mem_r=None, mem_t=None, uts=None, users=None, P, K, nR, depth=2,
                group=0, enc_entity=None, enc_relation=None, want_item_emb=True, want_sig=True):
    """mvin_score_small_fwd: the whole get_scores pass as ONE launch, on plain tensors (MVIN._score_small_native fills the same
    argument block for the model).  Feed: the per-pair lists ``mem_h`` / ``mem_r`` / ``mem_t`` (P int32 tensors [B, Nm] each) or
    ``uts`` [n_user, P, 3, Nm] int32 + ``users`` [B] int64.  ``adj_relation`` None: every relation reads as 0;
    ``enc_entity`` / ``enc_relation``: the duplicate-slot encoding (taken instead of the plain adjacency).  Every optional
    weight or bias may be None (the entry point's own rules decide which combinations it takes); ``depth`` 1 or 2; ``group`` pairs
    per workgroup (0: chosen from the batch); ``want_item_emb`` / ``want_sig`` False pass NULL for that output.
    -> (user_o [B, D], item_emb [B, D] | None, scores [B], sigmoid [B] | None)."""
    lib = _lib.load()
    _chk(entity_emb, F32, "entity_emb")
    for t, nm in ((adj_entity, "adj_entity"), (adj_relation, "adj_relation"), (enc_entity, "enc_entity"), (enc_relation, "enc_relation"),
                  (uts, "uts")):
        _chk(t, I32, nm)
    for t, nm in ((relation_kge, "relation_kge"), (h_set_w, "h_set_w"), (user_mlp_W, "user_mlp_W"), (user_mlp_b, "user_mlp_b"), (t0, "t0"),
                  (t1, "t1"), (W0, "W0"), (b0, "b0"), (W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2"), (A0, "A0"), (a0, "a0"), (A1, "A1"),
                  (a1, "a1"), (Wmix, "Wmix"), (bmix, "bmix")):
        _chk(t, F32, nm)
    _chk(items, torch.int64, "items"), _chk(users, torch.int64, "users")
    n_entity, D = entity_emb.shape
    B = items.shape[0]
    s = _lib.ScoreL2Args()
    s.entity_emb, s.adj_entity, s.adj_relation = _p(entity_emb), _p(adj_entity), _p(adj_relation)
    s.enc_entity, s.enc_relation = _p(enc_entity), _p(enc_relation)
    s.relation_kge, s.h_set_w, s.user_mlp_W, s.user_mlp_b, s.t0, s.t1 = (_p(t) for t in (relation_kge, h_set_w, user_mlp_W, user_mlp_b, t0, t1))
    s.W0, s.b0, s.W1, s.b1, s.W2, s.b2 = (_p(t) for t in (W0, b0, W1, b1, W2, b2))
    s.A0, s.a0, s.A1, s.a1, s.Wmix, s.bmix = (_p(t) for t in (A0, a0, A1, a1, Wmix, bmix))
    s.items = _p(items)
    hold = None
    if uts is not None:
        if users is None or uts.dim() != 4 or uts.shape[1] != max(1, P) or uts.shape[2] != 3:
            raise ValueError("uts [n_user, P, 3, Nm] needs users [B]")
        s.uts, s.users, s.n_user, Nm = _p(uts), _p(users), uts.shape[0], uts.shape[3]
    else:
        for lst, nm in ((mem_h, "mem_h"), (mem_r, "mem_r"), (mem_t, "mem_t")):
            if lst is None or len(lst) < P:
                raise ValueError(f"{nm}: P tensors [B, Nm] (or uts + users)")
            for t in lst[:P]:
                _chk(t, I32, nm)
        arr = C.c_void_p * P
        hold = tuple(arr(*[t.data_ptr() for t in lst[:P]]) for lst in (mem_h, mem_r, mem_t))
        s.mem_h, s.mem_r, s.mem_t = (C.addressof(h) for h in hold)
        Nm = mem_h[0].shape[1]
    dev = entity_emb.device
    user_o = torch.empty((B, D), dtype=F32, device=dev)
    item_emb = torch.empty((B, D), dtype=F32, device=dev) if want_item_emb else None
    scores = torch.empty(B, dtype=F32, device=dev)
    sig = torch.empty(B, dtype=F32, device=dev) if want_sig else None
    s.user_o, s.item_emb, s.scores, s.sig = _p(user_o), _p(item_emb), _p(scores), _p(sig)
    s.B, s.D, s.K, s.P, s.Nm, s.n_entity, s.n_relation, s.table_bf16, s.depth = B, D, K, P, Nm, n_entity, nR, 0, depth
    rc = lib.mvin_score_small_fwd(C.byref(s), int(group), _stream())
    del hold
    _lib.check(rc, "mvin_score_small_fwd")
    return user_o, item_emb, scores, sig


def gather_attn(table, adj_entity, adj_relation, node_ids, rel_score_t, self_vec, Wc, c_child,
                Wagg, bagg, B, N, K, D, want_probs=False):
    """mvin_gather_attn_fwd(_ex): deepest hop, children gathered from ``table`` (fp32 or bf16)
    through the adjacency of ``node_ids`` [B*N]; returns (out [B,N,D], probs [B,N,K] or None)."""
    lib = _lib.load()
    bf = _chk_table(table, "table")
    for t, dt, nm in ((adj_entity, I32, "adj_entity"),
                      (adj_relation, I32, "adj_relation"), (node_ids, I32, "node_ids"),
                      (rel_score_t, F32, "rel_score"), (self_vec, F32, "self_vec"), (Wc, F32, "Wc"),
                      (c_child, F32, "c_child"), (Wagg, F32, "Wagg"), (bagg, F32, "bagg")):
        _chk(t, dt, nm)
    out = torch.empty((B, N, D), dtype=F32, device=table.device)
    probs = torch.empty((B, N, K), dtype=F32, device=table.device) if want_probs else None
    _lib.check(lib.mvin_gather_attn_fwd_ex(_p(table), _p(adj_entity), _p(adj_relation), _p(node_ids),
                                           _p(rel_score_t), _p(self_vec), _p(Wc), _p(c_child), _p(Wagg),
                                           _p(bagg), B, N, K, D, table.shape[0], _p(out), _p(probs), None, None,
                                           bf, _stream()), "mvin_gather_attn_fwd_ex")
    return out, probs


def agg(self_vec, neigh, rel_ids, rel_score_t, Wagg, bagg, B, N, K, D, want_probs=False):
    """mvin_agg_fwd on materialised levels; ``rel_ids`` None with ``rel_score_t`` given means
    ``rel_score_t`` already holds one logit per child ([B*N*K])."""
    lib = _lib.load()
    for t, dt, nm in ((self_vec, F32, "self_vec"), (neigh, F32, "neigh"), (rel_ids, I32, "rel_ids"),
                      (rel_score_t, F32, "rel_score"), (Wagg, F32, "Wagg"), (bagg, F32, "bagg")):
        _chk(t, dt, nm)
    out = torch.empty((B, N, D), dtype=F32, device=self_vec.device)
    probs = torch.empty((B, N, K), dtype=F32, device=self_vec.device) if want_probs else None
    _lib.check(lib.mvin_agg_fwd(_p(self_vec), _p(neigh), _p(rel_ids), _p(rel_score_t), _p(Wagg),
                                _p(bagg), B, N, K, D, _p(out), _p(probs), _stream()), "mvin_agg_fwd")
    return out, probs


def ripple_attn(entity_emb, score_ids, rel_ids, value_ids, V, w, mode, out, out_offset, ldo, nR):
    """mvin_ripple_attn_fwd_ex: one ripple-set attention read per pair (fp32 or bf16 table), written into
    ``out`` (a [B, ldo] buffer) at column offset ``out_offset``."""
    lib = _lib.load()
    bf = _chk_table(entity_emb, "entity_emb")
    for t, dt, nm in ((score_ids, I32, "score_ids"),
                      (rel_ids, I32, "rel_ids"), (value_ids, I32, "value_ids"), (V, F32, "V"),
                      (w, F32, "w"), (out, F32, "out")):
        _chk(t, dt, nm)
    B, Nm = score_ids.shape
    D = entity_emb.shape[1]
    _lib.check(lib.mvin_ripple_attn_fwd_ex(_p(entity_emb), _p(score_ids), _p(rel_ids), _p(value_ids),
                                           _p(V), _p(w), mode, B, Nm, D, nR, _p(out, out_offset), ldo, bf,
                                           _stream()), "mvin_ripple_attn_fwd")
    return out


def gather_attn_l2_supported(D, K):
    return bool(_lib.load().mvin_gather_attn_l2_supported(D, K))


def probe_gather_l2(table, child_ids, grandchild_ids, K, sums=None):
    """mvin_probe_gather_l2: read the K child rows and K*K grandchild rows of every parent (id lists = levels 1 and 2
    of expand_ids) and add them up; returns sums [n_parents] (measurement aid, include/mvin_hip.h)."""
    bf = _chk_table(table, "table")
    _chk(child_ids, I32, "child_ids"), _chk(grandchild_ids, I32, "grandchild_ids")
    n = child_ids.numel() // K
    if grandchild_ids.numel() != n * K * K:
        raise ValueError("grandchild_ids must hold K*K ids per parent")
    if sums is None:
        sums = torch.empty(n, dtype=F32, device=table.device)
    else:
        _chk(sums, F32, "sums")
    _lib.check(_lib.load().mvin_probe_gather_l2(_p(table), _p(child_ids), _p(grandchild_ids), n, K, table.shape[1],
                                                table.shape[0], bf, _p(sums), _stream()), "mvin_probe_gather_l2")
    return sums


def gather_attn_l2_prj_supported(D, K, encoded, n_entity, n_relation):
    """Does mvin_gather_attn_l2_prj_fwd take these tables (encoded: the packed-tile kernel; plain: D = 32, K in {8, 16})?"""
    return bool(_lib.load().mvin_gather_attn_l2_prj_supported(D, K, int(bool(encoded)), n_entity, n_relation))


def gather_attn_l2_variant(D, K, n_parents, n_entity, want_probs=False, table_bf16=False):
    """0 = unsupported, 1 = symmetric fused kernel, 2 = role-split pipeline, 3 / 4 = wave-per-parent kernels (include/mvin_hip.h)."""
    return int(_lib.load().mvin_gather_attn_l2_variant_ex(D, K, n_parents, n_entity, int(bool(want_probs)), int(bool(table_bf16))))


def gather_attn_l2(table, adj_entity, adj_relation, parent_ids, t0, t1, W1, W2, b1, b2, q, A0, a0,
                   B, parents_per_pair, K, D, nR, want_probs=False):
    """mvin_gather_attn_l2_fwd: the two deepest levels in one pass.  ``parent_ids``: int32, or int64 read in place
    (mvin_gather_attn_l2_fwd_i64: the batch's item ids at tree depth 2).  Returns
    (nagg0 [P,D], nagg1 [P,D], probs_parent [P,K] | None, probs_child [P*K,K] | None)."""
    lib = _lib.load()
    bf = _chk_table(table, "table")
    for t, dt, nm in ((adj_entity, I32, "adj_entity"), (adj_relation, I32, "adj_relation"),
                      (parent_ids, torch.int64 if parent_ids.dtype == torch.int64 else I32, "parent_ids"), (t0, F32, "t0"), (t1, F32, "t1"), (W1, F32, "W1"),
                      (W2, F32, "W2"), (b1, F32, "b1"), (b2, F32, "b2"), (q, F32, "q"), (A0, F32, "A0"),
                      (a0, F32, "a0")):
        _chk(t, dt, nm)
    P = B * parents_per_pair
    dev = table.device
    nagg0 = torch.empty((P, D), dtype=F32, device=dev)
    nagg1 = torch.empty((P, D), dtype=F32, device=dev)
    pp = torch.empty((P, K), dtype=F32, device=dev) if want_probs else None
    pc = torch.empty((P * K, K), dtype=F32, device=dev) if want_probs else None
    fn = lib.mvin_gather_attn_l2_fwd_i64 if parent_ids.dtype == torch.int64 else lib.mvin_gather_attn_l2_fwd
    _lib.check(fn(_p(table), _p(adj_entity), _p(adj_relation), _p(parent_ids), _p(t0),
                  _p(t1), _p(W1), _p(W2), _p(b1), _p(b2), _p(q), _p(A0), _p(a0), B,
                  parents_per_pair, K, D, table.shape[0], nR, _p(nagg0), _p(nagg1),
                  _p(pp), _p(pc), bf, _stream()), "mvin_gather_attn_l2_fwd")
    return nagg0, nagg1, pp, pc


def encode_adjacency_supported(D, K):
    """The packed-tile fused kernel (mvin_gather_attn_l2_enc_fwd) exists for this shape."""
    return bool(_lib.load().mvin_gather_attn_l2_enc_supported(D, K))


def encode_adjacency(adj_entity, adj_relation):
    """mvin_encode_adjacency: the duplicate-slot encoding of a sampled adjacency (include/mvin_hip.h) ->
    (enc_entity [nE,K] int32, enc_relation [nE,K] int32, cnt [nE] int32 = distinct slots per row)."""
    _chk(adj_entity, I32, "adj_entity"), _chk(adj_relation, I32, "adj_relation")
    nE, K = adj_entity.shape
    enc_e, enc_r = torch.empty_like(adj_entity), torch.empty_like(adj_entity)
    cnt = torch.empty(nE, dtype=I32, device=adj_entity.device)
    _lib.check(_lib.load().mvin_encode_adjacency(_p(adj_entity), _p(adj_relation), nE, K, _p(cnt), _p(enc_e), _p(enc_r),
                                                 _stream()), "mvin_encode_adjacency")
    return enc_e, enc_r, cnt


def gather_attn_l2_enc(table, enc_entity, enc_relation, parent_ids, t0, t1, W1, W2, b1, b2, q, A0, a0,
                       B, parents_per_pair, K, D, nR):
    """mvin_gather_attn_l2_enc_fwd: gather_attn_l2 over the duplicate-slot encoding (packed tiles; no attention
    outputs).  Returns (nagg0 [P,D], nagg1 [P,D])."""
    lib = _lib.load()
    bf = _chk_table(table, "table")
    for t, dt, nm in ((enc_entity, I32, "enc_entity"), (enc_relation, I32, "enc_relation"),
                      (parent_ids, torch.int64 if parent_ids.dtype == torch.int64 else I32, "parent_ids"), (t0, F32, "t0"),
                      (t1, F32, "t1"), (W1, F32, "W1"), (W2, F32, "W2"), (b1, F32, "b1"), (b2, F32, "b2"), (q, F32, "q"),
                      (A0, F32, "A0"), (a0, F32, "a0")):
        _chk(t, dt, nm)
    P = B * parents_per_pair
    nagg0 = torch.empty((P, D), dtype=F32, device=table.device)
    nagg1 = torch.empty((P, D), dtype=F32, device=table.device)
    _lib.check(lib.mvin_gather_attn_l2_enc_fwd(_p(table), _p(enc_entity), _p(enc_relation), _p(parent_ids),
                                               int(parent_ids.dtype == torch.int64), _p(t0), _p(t1), _p(W1), _p(W2), _p(b1),
                                               _p(b2), _p(q), _p(A0), _p(a0), B, parents_per_pair, K, D, table.shape[0], nR,
                                               _p(nagg0), _p(nagg1), bf, _stream()), "mvin_gather_attn_l2_enc_fwd")
    return nagg0, nagg1


def project_rows(src, W1, W2, b1=None, b2=None):
    """mvin_project_rows: [2, rows, D] = (src . W1 (+ b1), src . W2 (+ b2)) -- the two projections of the levels the fused
    two-level kernel gathers, of the entity table's rows or of the pairs' query vectors."""
    lib = _lib.load()
    for t, nm in ((src, "src"), (W1, "W1"), (W2, "W2"), (b1, "b1"), (b2, "b2")):
        _chk(t, F32, nm)
    rows, D = src.shape
    out = torch.empty((2, rows, D), dtype=F32, device=src.device)
    _lib.check(lib.mvin_project_rows(_p(src), rows, D, _p(W1), _p(W2), _p(b1), _p(b2), _p(out), _stream()), "mvin_project_rows")
    return out


def project_tables(entity_emb, W1, W2, b1, b2, A0, a0, K, attention, out=None):
    """mvin_project_tables: the workspace of the projected-tables form -- E.W1 | E.W1.A0 | E.W2.A0 and the per-call parameter
    block -- from the CURRENT parameters.  ``attention``: whether the relation logits t0 will be given to the gather."""
    lib = _lib.load()
    for t, nm in ((entity_emb, "entity_emb"), (W1, "W1"), (W2, "W2"), (b1, "b1"), (b2, "b2"), (A0, "A0"), (a0, "a0")):
        _chk(t, F32, nm)
    nE, D = entity_emb.shape
    n = lib.mvin_project_tables_elems(nE, D)
    if out is None:
        out = torch.empty((n,), dtype=F32, device=entity_emb.device)
    elif out.numel() != n or out.dtype != F32 or not out.is_contiguous():
        raise ValueError("project_tables: workspace of mvin_project_tables_elems floats expected")
    _lib.check(lib.mvin_project_tables(_p(entity_emb), _p(W1), _p(W2), _p(b1), _p(b2), _p(A0), _p(a0), 1 if attention else 0, K, nE, D,
                                       _p(out), _stream()), "mvin_project_tables")
    return out


def gather_attn_l2_wpp_supported(D, K):
    """The shapes the wave-per-parent kernel over projected tables takes (it is the one that honours ``order``)."""
    return D == 64 and K in (16, 32) and os.environ.get("MVIN_L2_WPP", "1") != "0"


def order_by_key(keys, ws=None, out=None):
    """mvin_order_by_key: a permutation of 0 .. B-1 (int32) in which equal keys (int64 / int32 ids) are neighbours -- a partition by
    the key's low bits, not a sort; the order inside a bucket is unspecified."""
    lib = _lib.load()
    B = keys.shape[0]
    _chk(keys, torch.int64 if keys.dtype == torch.int64 else I32, "keys")
    n = lib.mvin_order_by_key_ws_elems(B)
    if ws is None or ws.numel() < n:
        ws = torch.empty((n,), dtype=I32, device=keys.device)
    if out is None:
        out = torch.empty((B,), dtype=I32, device=keys.device)
    k64, k32 = (_p(keys), None) if keys.dtype == torch.int64 else (None, _p(keys))
    _lib.check(lib.mvin_order_by_key(k64, k32, B, _p(ws), _p(out), _stream()), "mvin_order_by_key")
    return out


def topk_rows_supported(k):
    return bool(_lib.load().mvin_topk_rows_supported(int(k)))


def topk_rows(scores, k, cand_ids=None, col_offset=0, excl=None, carry=None, out=None):
    """mvin_topk_rows: the ``k`` best eligible candidates of every row of ``scores`` ([rows, n] f32; rows may be strided, columns
    must be dense), higher score first, ties by position (carry entries first, then column order) -- the reference's stable
    ``sorted(..., reverse=True)``.  ``cand_ids`` [n] int32: item id of each column (None: ``col_offset + j``); ``excl``: a
    ``(ptr int64 [rows+1], ids int32)`` CSR of item ids excluded per row, each row ascending; ``carry``: ``(ids, vals)`` [rows, k],
    a running top-K of earlier column blocks (id -1 = padding); ``out``: ``(ids, vals)`` to write, may be ``carry`` itself.
    Returns ``(ids int32 [rows, k], vals f32 [rows, k])``; short rows are padded with id -1, value -inf."""
    lib = _lib.load()
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise _lib.MvinHipError("scores: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if scores.dtype != F32:
        raise TypeError(f"scores: expected {F32}, got {scores.dtype}")
    if scores.dim() != 2 or (scores.shape[1] > 1 and scores.stride(1) != 1) or scores.stride(0) < scores.shape[1]:
        raise ValueError("scores: expected a [rows, n] tensor with dense rows")
    k = int(k)
    if not topk_rows_supported(k):
        raise ValueError(f"k={k}: mvin_topk_rows takes 1 <= k <= 1024")
    rows, n = scores.shape
    dev = scores.device
    if cand_ids is not None:
        _chk(cand_ids, I32, "cand_ids")
        if cand_ids.numel() != n:
            raise ValueError(f"cand_ids: {cand_ids.numel()} ids for {n} columns")
    ptr = ids = None
    if excl is not None:
        ptr, ids = excl
        _chk(ptr, torch.int64, "excl ptr")
        _chk(ids, I32, "excl ids")
        if ptr.numel() != rows + 1:
            raise ValueError(f"excl ptr: {ptr.numel()} entries for {rows} rows")
    cid = cval = None
    if carry is not None:
        cid, cval = carry
        _chk(cid, I32, "carry ids")
        _chk(cval, F32, "carry vals")
        if tuple(cid.shape) != (rows, k) or tuple(cval.shape) != (rows, k):
            raise ValueError(f"carry: expected [{rows}, {k}]")
    if out is None:
        out = (torch.empty((rows, k), dtype=I32, device=dev), torch.empty((rows, k), dtype=F32, device=dev))
    oid, oval = out
    _chk(oid, I32, "out ids")
    _chk(oval, F32, "out vals")
    if tuple(oid.shape) != (rows, k) or tuple(oval.shape) != (rows, k):
        raise ValueError(f"out: expected [{rows}, {k}]")
    nws = lib.mvin_topk_rows_ws_bytes(rows, n, k)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    ld = scores.stride(0) if rows > 1 else n
    ids_p = None if ids is None or ids.numel() == 0 else _p(ids)
    if ptr is not None and ids_p is None:
        ids_p = _p(ptr)                         # every row empty: any valid pointer, nothing is read through it
    _lib.check(lib.mvin_topk_rows(_p(scores) if n > 0 else None, rows, n, ld, _p(cand_ids), int(col_offset), _p(ptr), ids_p,
                                  _p(cid), _p(cval), k, _p(ws), _p(oid), _p(oval), _stream()), "mvin_topk_rows")
    return oid, oval


CTR_SEG_CAP = 16384          # MVIN_CTR_SEG_CAP: the longest segment mvin_ctr_counts handles in one workgroup, without workspace
CTR_COLUMNS = ("n_pos", "n_neg", "tp", "fp", "u2", "bad")


class UndefinedMetricWarning(UserWarning):
    """A metric is undefined for some segments (sklearn's warning of the same name and meaning)."""


def _ctr_rows(t, name, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name}: expected a [segments, seg_len] tensor with dense rows")


def ctr_counts(scores, labels, seg_len, out=None):
    """mvin_ctr_counts: the exact CTR counts of every segment, an int64 [S, 6] device tensor (columns ``CTR_COLUMNS``: label
    counts, tp / fp of ``score >= 0.5``, twice the Mann-Whitney U, non-finite scores plus labels other than 0 / 1).
    ``scores`` f32 and ``labels`` int32 are either 1-D of S * seg_len pairs (contiguous) or [S, seg_len] with dense rows and
    the same row stride.  Enqueues only: no synchronisation, no copy to the host (ctr_metrics_from_counts reads the result)."""
    lib = _lib.load()
    seg_len = int(seg_len)
    if seg_len < 1:
        raise ValueError(f"seg_len={seg_len}: expected >= 1")
    if isinstance(scores, torch.Tensor) and scores.dim() == 1:
        if scores.numel() % seg_len:
            raise ValueError(f"scores: {scores.numel()} pairs are not whole segments of {seg_len}")
        _chk(scores, F32, "scores")
        scores = scores.view(-1, seg_len)
    if isinstance(labels, torch.Tensor) and labels.dim() == 1:
        _chk(labels, I32, "labels")
        labels = labels.view(-1, seg_len) if labels.numel() % seg_len == 0 else labels
    _ctr_rows(scores, "scores", F32)
    _ctr_rows(labels, "labels", I32)
    if tuple(scores.shape) != tuple(labels.shape) or scores.shape[1] != seg_len:
        raise ValueError(f"scores {tuple(scores.shape)} and labels {tuple(labels.shape)}: expected [S, {seg_len}] both")
    S = scores.shape[0]
    ld = scores.stride(0) if S > 1 else seg_len
    if S > 1 and labels.stride(0) != ld:
        raise ValueError(f"labels: row stride {labels.stride(0)}, scores: {ld}; the two must share one layout")
    dev = scores.device
    if out is None:
        out = torch.empty((S, 6), dtype=torch.int64, device=dev)
    _chk(out, torch.int64, "out")
    if tuple(out.shape) != (S, 6):
        raise ValueError(f"out: expected [{S}, 6]")
    if S == 0:
        return out
    nws = lib.mvin_ctr_counts_ws_bytes(S, seg_len)
    if nws < 0:
        _lib.check(int(nws), "mvin_ctr_counts_ws_bytes")
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    _lib.check(lib.mvin_ctr_counts(_p(scores), _p(labels), S, seg_len, ld, _p(ws), _p(out), _stream()), "mvin_ctr_counts")
    return out


def ctr_metrics_from_counts(counts):
    """Per-segment ``(auc, acc, f1)`` float64 arrays from ctr_counts rows (a host array, [S, 6] or [6]), by sklearn 1.7's
    conventions: ``auc = u2 / (2 n_pos n_neg)`` -- NaN for a segment with one class only, with ONE UndefinedMetricWarning per
    call naming how many segments; ``acc = (tp + n_neg - fp) / n``; ``f1 = 2 tp / (2 tp + fp + fn)``, 0.0 where that
    denominator is 0.  A segment with ``bad > 0`` (a NaN or infinite score, or a label other than 0 / 1, which sklearn rejects)
    raises ValueError."""
    import warnings
    import numpy as np
    c = np.asarray(counts)
    if c.ndim == 1:
        c = c.reshape(1, -1)
    if c.ndim != 2 or c.shape[1] != 6:
        raise ValueError(f"counts: expected [S, 6], got {c.shape}")
    c = c.astype(np.int64, copy=False)
    n_pos, n_neg, tp, fp, u2, bad = (c[:, q] for q in range(6))
    if (bad > 0).any():
        s = int(np.flatnonzero(bad > 0)[0])
        raise ValueError(f"segment {s}: {int(bad[s])} non-finite score(s) or label(s) other than 0 / 1")
    n = (n_pos + n_neg).astype(np.float64)
    one = (n_pos == 0) | (n_neg == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = np.where(one, np.nan, u2.astype(np.float64) / (2.0 * n_pos.astype(np.float64) * n_neg.astype(np.float64)))
        acc = (tp + n_neg - fp).astype(np.float64) / n
        den = (2 * tp + fp + (n_pos - tp)).astype(np.float64)
        f1 = np.where(den > 0, (2 * tp).astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)
    if one.any():
        warnings.warn(f"Only one class is present in {int(one.sum())} of {c.shape[0]} segment(s): ROC AUC is not defined there "
                      "(NaN)", UndefinedMetricWarning, stacklevel=2)
    return auc, acc, f1


PLACEMENT_COUNTS = ("n_pos", "n_neg", "u2", "bad")


def ctr_placements(scores, labels, out=None):
    """mvin_ctr_placements: every row's placement among the valid rows of the other class.  ``scores`` f32 [n] and ``labels``
    int32 [n] (contiguous device tensors, ONE population).  Returns ``(place int64 [n], counts int64 [4])`` on the device
    (``out``: the same two to write into): ``place[i] = 2 #{other class below} + #{other class equal}`` with ctr_counts' image
    and tie rule, -1 for a row with a non-finite score or a label other than 0 / 1; ``counts`` = ``PLACEMENT_COUNTS``, with
    ``u2`` the sum of the positives' placements -- ctr_counts' u2.  All integers, the same on every launch.  Enqueues only."""
    lib = _lib.load()
    for t, name in ((scores, "scores"), (labels, "labels")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if scores.dtype != F32:
        raise TypeError(f"scores: expected {F32}, got {scores.dtype}")
    if labels.dtype != I32:
        raise TypeError(f"labels: expected {I32}, got {labels.dtype}")
    if scores.dim() != 1 or labels.dim() != 1 or scores.shape != labels.shape or not scores.is_contiguous() or not labels.is_contiguous():
        raise ValueError(f"scores {tuple(scores.shape)} and labels {tuple(labels.shape)}: expected two contiguous [n] tensors")
    n = scores.numel()
    if not 1 <= n < 1 << 31:
        raise ValueError(f"n={n}: mvin_ctr_placements takes 1 <= n < 2^31 rows")
    dev = scores.device
    if out is None:
        out = (torch.empty((n,), dtype=torch.int64, device=dev), torch.empty((4,), dtype=torch.int64, device=dev))
    if len(out) != 2:
        raise ValueError("out: expected (place, counts)")
    place, counts = _chk(out[0], torch.int64, "out place"), _chk(out[1], torch.int64, "out counts")
    if place is None or counts is None or tuple(place.shape) != (n,) or tuple(counts.shape) != (4,):
        raise ValueError(f"out: expected place int64 [{n}] and counts int64 [4]")
    nws = lib.mvin_ctr_placements_ws_bytes(n)
    if nws < 0:
        _lib.check(int(nws), "mvin_ctr_placements_ws_bytes")
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    _lib.check(lib.mvin_ctr_placements(_p(scores), _p(labels), n, _p(ws), _p(place), _p(counts), _stream()), "mvin_ctr_placements")
    return place, counts


TAIL_COUNTS = ("n_pos", "n_neg", "bad")
OPERATING_CRITERIA = ("f1", "acc", "youden")          # the rows of ctr_operating_points' thr and cells


def _curve_rows(scores, labels, who, allow_empty=False):
    """The checks ctr_tails, ctr_operating_points and ctr_threshold_counts share: ValueError for anything but two contiguous device
    tensors f32 [n] / int32 [n] of one population within the row limit; returns n."""
    for t, name, dt in ((scores, "scores", F32), (labels, "labels", I32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{who}: {name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
        if t.dtype != dt:
            raise ValueError(f"{who}: {name}: expected {dt}, got {t.dtype}")
    if scores.dim() != 1 or labels.dim() != 1 or scores.shape != labels.shape or not scores.is_contiguous() or not labels.is_contiguous():
        raise ValueError(f"{who}: scores {tuple(scores.shape)} and labels {tuple(labels.shape)}: expected two contiguous [n] tensors")
    if labels.device != scores.device:
        raise ValueError(f"{who}: scores on {scores.device}, labels on {labels.device}")
    n = scores.numel()
    if not (0 if allow_empty else 1) <= n < 1 << 31:
        raise ValueError(f"n={n}: {who} takes {'0' if allow_empty else '1'} <= n < 2^31 rows")
    return n


def _curve_out(t, name, dtype, shape, dev, who):
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{who}: {name}: expected a contiguous {dtype} {list(shape)} tensor on {dev}")
    return t


def ctr_tails(scores, labels, out=None):
    """mvin_ctr_tails: every row's tail counts.  ``scores`` f32 [n] and ``labels`` int32 [n] (contiguous device tensors, ONE
    population).  Returns ``(tails int32 [n, 2], counts int64 [3])`` on the device (``out``: the same two to write into):
    ``tails[i] = (tp, fp)`` = the valid positives / negatives whose score is >= row i's own (ctr_counts' image: -0.0 equals +0.0),
    i.e. the confusion cells at the cut "row i's score"; (-1, -1) for a row with a non-finite score or a label other than 0 / 1;
    ``counts`` = ``TAIL_COUNTS``.  All integers, the same on every launch.  Enqueues only.  ValueError for anything but such
    tensors."""
    lib = _lib.load()
    n = _curve_rows(scores, labels, "ctr_tails")
    dev = scores.device
    if out is None:
        out = (torch.empty((n, 2), dtype=I32, device=dev), torch.empty((3,), dtype=torch.int64, device=dev))
    if len(out) != 2:
        raise ValueError("ctr_tails: out: expected (tails, counts)")
    tails = _curve_out(out[0], "out tails", I32, (n, 2), dev, "ctr_tails")
    counts = _curve_out(out[1], "out counts", torch.int64, (3,), dev, "ctr_tails")
    nws = lib.mvin_ctr_tails_ws_bytes(n)
    if nws < 0:
        _lib.check(int(nws), "mvin_ctr_tails_ws_bytes")
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    _lib.check(lib.mvin_ctr_tails(_p(scores), _p(labels), n, _p(ws), _p(tails), _p(counts), _stream()), "mvin_ctr_tails")
    return tails, counts


def ctr_operating_points(tails, scores, labels, max_groups=0):
    """mvin_ctr_operating_points: the best cuts of a split and its average-precision sum, from ctr_tails' ``tails`` of the same
    ``scores`` and ``labels``.  Returns device tensors ``(thr f32 [3], cells int64 [3, 2], ap_sum f64 [1])``: per criterion of
    ``OPERATING_CRITERIA`` the cut that maximises it over every valid row's own score and the empty cut (+inf), compared as
    exact integers, ties to the higher cut; its (tp, fp); and the sum of tp / (tp + fp) over the valid positives in one fixed
    order (average_precision_from_sum divides it by n_pos).  The same bits for every ``max_groups`` (0 automatic, else a cap on
    the workgroups).  Enqueues only.  ValueError for anything but matching device tensors."""
    lib = _lib.load()
    n = _curve_rows(scores, labels, "ctr_operating_points")
    dev = scores.device
    _curve_out(tails, "tails", I32, (n, 2), dev, "ctr_operating_points")
    max_groups = int(max_groups)
    if max_groups < 0:
        raise ValueError(f"max_groups={max_groups}: expected >= 0")
    thr = torch.empty((3,), dtype=F32, device=dev)
    cells = torch.empty((3, 2), dtype=torch.int64, device=dev)
    ap_sum = torch.empty((1,), dtype=torch.float64, device=dev)
    nws = lib.mvin_ctr_operating_points_ws_bytes(n)
    if nws < 0:
        _lib.check(int(nws), "mvin_ctr_operating_points_ws_bytes")
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    _lib.check(lib.mvin_ctr_operating_points(_p(tails), _p(scores), _p(labels), n, _p(ws), max_groups, _p(thr), _p(cells), _p(ap_sum),
                                             _stream()), "mvin_ctr_operating_points")
    return thr, cells, ap_sum


def ctr_threshold_counts_max():
    """mvin_ctr_threshold_counts_max: the thresholds one mvin_ctr_threshold_counts call takes (4096)."""
    return int(_lib.load().mvin_ctr_threshold_counts_max())


def ctr_threshold_counts(scores, labels, thresholds, max_groups=0):
    """mvin_ctr_threshold_counts: the confusion cells of a split at many cuts at once.  ``thresholds`` f32 [T] on the device, in
    any order, duplicates allowed.  Returns device tensors ``(out int64 [T, 2], counts int64 [3])``: ``out[t] = (tp, fp)`` = the
    valid positives / negatives with ``score >= thresholds[t]`` compared in f32 (a NaN threshold: (0, 0)), ``counts`` =
    ``TAIL_COUNTS``.  More than ctr_threshold_counts_max() thresholds are cut into calls.  Integers only, the same bits for
    every ``max_groups``.  Enqueues only.  ValueError for wrong dtypes, devices or shapes."""
    lib = _lib.load()
    who = "ctr_threshold_counts"
    n = _curve_rows(scores, labels, who, allow_empty=True)
    dev = scores.device
    if not isinstance(thresholds, torch.Tensor) or thresholds.device != dev or thresholds.dtype != F32 or thresholds.dim() != 1 \
            or thresholds.numel() < 1 or not thresholds.is_contiguous():
        raise ValueError(f"{who}: thresholds: expected a contiguous {F32} [T] tensor on {dev}, T >= 1")
    max_groups = int(max_groups)
    if max_groups < 0:
        raise ValueError(f"max_groups={max_groups}: expected >= 0")
    T, step = thresholds.numel(), ctr_threshold_counts_max()
    out = torch.empty((T, 2), dtype=torch.int64, device=dev)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        _lib.check(lib.mvin_ctr_threshold_counts(_p(scores) if n else None, _p(labels) if n else None, n, _p(thresholds[t0:t1]), t1 - t0,
                                                 max_groups, _p(out[t0:t1]), _p(counts), _stream()), "mvin_ctr_threshold_counts")
    return out, counts


def average_precision_from_sum(ap_sum, counts):
    """The average precision ``ap_sum / n_pos`` in float64 from ctr_operating_points' sum and ctr_tails' counts (host values);
    NaN when there is no valid positive.  sklearn's average_precision_score on the valid rows: the sum of the positives'
    precisions at their own scores equals its sum of (R_k - R_(k-1)) P_k over the distinct thresholds."""
    m = int(np.asarray(counts).reshape(-1)[0])
    s = np.float64(np.asarray(ap_sum, dtype=np.float64).reshape(-1)[0])
    return float(s / np.float64(m)) if m > 0 else float("nan")


def operating_point_metrics(tp, fp, m, n0):
    """The metrics of the cut with confusion cells ``tp``, ``fp`` on ``m`` positives and ``n0`` negatives (Python ints), in
    float64 by ctr_metrics_from_counts' conventions: ``acc = (tp + n0 - fp) / n`` (NaN for no rows), ``f1 = 2 tp / (2 tp + fp +
    fn)`` and ``precision = tp / (tp + fp)`` -- 0.0 where that denominator is 0 -- ``recall = tp / m`` and ``fpr = fp / n0`` --
    NaN for an empty class -- and ``youden = recall - fpr``."""
    tp, fp, m, n0 = int(tp), int(fp), int(m), int(n0)
    f = np.float64
    nan = float("nan")
    den = 2 * tp + fp + (m - tp)
    recall = float(f(tp) / f(m)) if m > 0 else nan
    fpr = float(f(fp) / f(n0)) if n0 > 0 else nan
    return {"acc": float(f(tp + n0 - fp) / f(m + n0)) if m + n0 > 0 else nan,
            "f1": float(f(2 * tp) / f(den)) if den > 0 else 0.0,
            "precision": float(f(tp) / f(tp + fp)) if tp + fp > 0 else 0.0,
            "recall": recall, "fpr": fpr, "youden": recall - fpr}


def curves_from_counts(thresholds, out, counts):
    """The ROC and PR points at ctr_threshold_counts' thresholds (host arrays [T], [T, 2], [3]), float64, in the thresholds' own
    order: ``{"roc": {"fpr", "tpr"}, "pr": {"precision", "recall"}}`` with tpr = recall = tp / n_pos and fpr = fp / n_neg (NaN
    for an empty class) and precision = tp / (tp + fp), 1.0 where nothing is predicted positive (precision_recall_curve's last
    point)."""
    thr = np.asarray(thresholds).reshape(-1)
    c = np.asarray(out).astype(np.int64)
    ct = np.asarray(counts).reshape(-1)
    if c.ndim != 2 or c.shape != (thr.size, 2) or ct.size != 3:
        raise ValueError(f"expected thresholds [T], out [T, 2] and counts [3], got {thr.shape}, {c.shape}, {ct.shape}")
    m, n0 = int(ct[0]), int(ct[1])
    tp, fp = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = tp / np.float64(m) if m > 0 else np.full(thr.size, np.nan)
        fpr = fp / np.float64(n0) if n0 > 0 else np.full(thr.size, np.nan)
        pred = tp + fp
        precision = np.where(pred > 0, tp / np.where(pred > 0, pred, 1.0), 1.0)
    return {"roc": {"fpr": fpr, "tpr": tpr}, "pr": {"precision": precision, "recall": tpr.copy()}}


RANK_RESAMPLE_WORDS = 12                              # out's words before the fixed cuts: M, N, u2, 3 x (tp, fp, pos)
RANK_RESAMPLE_MULT_BYTES = 256 << 20                  # ctr_rank_resample's default budget for one call's multiplicities and workspace


def resample_multiplicities(n_units, n_rep, seed=1, first=0, device=None, out=None):
    """mvin_resample_multiplicities: ``mult`` int32 [n_rep, n_units] on the device, ``mult[r - first][i]`` = how often replicate r
    of ``seed`` draws unit i -- the histogram of resample_sums' bootstrap draws over ``n_units`` rows, so replicate r here
    resamples the units replicate r of a resample_sums call over a table of ``n_units`` rows does.  Every row sums to n_units.
    ``out``: an int32 [n_rep, >= n_units] tensor with dense rows to write into (columns beyond n_units are left alone).
    Enqueues only."""
    lib = _lib.load()
    n_units, n_rep, seed, first = int(n_units), int(n_rep), int(seed), int(first)
    if not 0 <= n_units < 1 << 31 or n_rep < 0 or first < 0:
        raise ValueError(f"n_units={n_units} n_rep={n_rep} first={first}: expected 0 <= n_units < 2^31 and n_rep, first >= 0")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed}: expected an unsigned 64-bit value")
    if out is None:
        out = torch.empty((n_rep, n_units), dtype=I32, device=device if device is not None else "cuda")
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != I32 or out.dim() != 2 or out.shape[0] != n_rep \
            or out.shape[1] < n_units or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"resample_multiplicities: out: expected a device int32 [{n_rep}, >= {n_units}] tensor with dense rows")
    ld = out.stride(0) if n_rep > 1 else max(out.shape[1], 1)
    if ld < out.shape[1]:
        raise ValueError("resample_multiplicities: out: rows overlap")
    if n_rep and n_units:
        _lib.check(lib.mvin_resample_multiplicities(n_units, C.c_uint64(seed), first, n_rep, _p(out), ld, _stream()),
                   "mvin_resample_multiplicities")
    return out[:, :n_units]


def ctr_rank_image(tails, labels, units=None):
    """mvin_ctr_rank_image: the split in descending score order, from ctr_tails' ``tails`` int32 [n, 2] and ``labels`` int32 [n].
    ``units`` int32 [n] names every row's sampling unit (its cluster); None: the row is its own unit.  Returns device tensors
    ``(pos_row int32 [n], image int32 [n, 2])``: the row at every position and (its unit, info) with info bit 0 = the label and
    bit 1 = the last position of a tie group; the positions behind the valid rows hold -1 and (-1, 0).  Which row of a tie group
    sits where inside it is not specified (nothing downstream depends on it).  Enqueues only.  ValueError for anything but
    matching contiguous device tensors."""
    lib = _lib.load()
    who = "ctr_rank_image"
    if not isinstance(tails, torch.Tensor) or not tails.is_cuda or tails.dtype != I32 or tails.dim() != 2 or tails.shape[1] != 2 \
            or not tails.is_contiguous():
        raise ValueError(f"{who}: tails: expected a contiguous device int32 [n, 2] tensor")
    n, dev = tails.shape[0], tails.device
    if not 1 <= n < 1 << 31:
        raise ValueError(f"n={n}: {who} takes 1 <= n < 2^31 rows")
    _curve_out(labels, "labels", I32, (n,), dev, who)
    if units is not None:
        _curve_out(units, "units", I32, (n,), dev, who)
    pos_row = torch.empty((n,), dtype=I32, device=dev)
    image = torch.empty((n, 2), dtype=I32, device=dev)
    ws = torch.empty((int(lib.mvin_ctr_rank_image_ws_bytes(n)),), dtype=torch.uint8, device=dev)
    _lib.check(lib.mvin_ctr_rank_image(_p(tails), _p(labels), _p(units), n, _p(ws), _p(pos_row), _p(image), _stream()),
               "mvin_ctr_rank_image")
    return pos_row, image


def ctr_rank_resample_max_cuts():
    """mvin_ctr_rank_resample_max_cuts: the fixed cuts one mvin_ctr_rank_resample call takes (64)."""
    return int(_lib.load().mvin_ctr_rank_resample_max_cuts())


def ctr_rank_resample(image, n_units=None, n_rep=0, seed=1, first=0, cut_pos=None, mult=None, max_groups=0, budget_bytes=None):
    """mvin_ctr_rank_resample over ctr_rank_image's ``image``: per replicate the weighted class totals, twice the weighted
    Mann-Whitney U, the best cut by F1 / accuracy / Youden as (tp, fp, pos) and the cells (TP, FP) above the fixed cuts
    ``cut_pos`` (positions, a list of ints or an int64 tensor), plus the average-precision sum.  Three forms:
      * ``n_units=None``: the observed split (every weight 1), one replicate;
      * ``mult`` int32 [R, n_units] on the device: these multiplicities;
      * otherwise the replicates ``first .. first + n_rep - 1`` of ``seed`` (resample_multiplicities), cut into calls so that one
        call's multiplicities and workspace stay within ``budget_bytes`` (RANK_RESAMPLE_MULT_BYTES) -- the rule makes that
        bit-neutral.
    Returns device tensors ``(out int64 [R, 12 + 2 n_cuts], ap_sum f64 [R])``; a replicate whose weights sum to 2^31 or more has
    -1 behind its totals and NaN.  The same bits for every ``max_groups``.  Enqueues only."""
    lib = _lib.load()
    who = "ctr_rank_resample"
    if isinstance(image, (list, tuple)):                    # several splits' images of the SAME units: one multiplicity table
        if n_units is None or mult is not None or not image:
            raise ValueError(f"{who}: a list of images takes n_units and the seeded form")
        if any(not isinstance(t, torch.Tensor) or t.shape != image[0].shape or t.device != image[0].device for t in image):
            raise ValueError(f"{who}: the images of a list must have one shape and one device")
        n_rep, first = int(n_rep), int(first)
        if n_rep < 0 or first < 0:
            raise ValueError(f"n_rep={n_rep} first={first}: expected values >= 0")
        budget = RANK_RESAMPLE_MULT_BYTES if budget_bytes is None else int(budget_bytes)
        n0 = image[0].shape[0]
        per_rep = 4 * max(int(n_units), 1) + max(int(lib.mvin_ctr_rank_resample_ws_bytes(n0, 1)), 0)
        step = max(1, budget // per_rep)
        parts = [[] for _ in image]
        buf = torch.empty((min(step, n_rep), max(int(n_units), 1)), dtype=I32, device=image[0].device) if n_rep else None
        for r0 in range(0, n_rep, step):
            R = min(step, n_rep - r0)
            resample_multiplicities(n_units, R, seed=seed, first=first + r0, out=buf[:R])
            for k, im in enumerate(image):
                parts[k].append(ctr_rank_resample(im, n_units=n_units, cut_pos=cut_pos, mult=buf[:R], max_groups=max_groups))
        if not n_rep:
            return [ctr_rank_resample(im, n_units=n_units, n_rep=0, cut_pos=cut_pos) for im in image]
        return [(torch.cat([o for o, _ in p]), torch.cat([a for _, a in p])) for p in parts]
    if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != I32 or image.dim() != 2 or image.shape[1] != 2 \
            or not image.is_contiguous():
        raise ValueError(f"{who}: image: expected a contiguous device int32 [n, 2] tensor")
    n, dev = image.shape[0], image.device
    if not 1 <= n < 1 << 31:
        raise ValueError(f"n={n}: {who} takes 1 <= n < 2^31 positions")
    max_groups = int(max_groups)
    if max_groups < 0:
        raise ValueError(f"max_groups={max_groups}: expected >= 0")
    if cut_pos is None:
        cut_pos = []
    if not isinstance(cut_pos, torch.Tensor):
        cut_pos = torch.tensor([int(q) for q in cut_pos], dtype=torch.int64, device=dev)
    if cut_pos.device != dev or cut_pos.dtype != torch.int64 or cut_pos.dim() != 1 or not cut_pos.is_contiguous():
        raise ValueError(f"{who}: cut_pos: expected ints or a contiguous int64 [n_cuts] tensor on {dev}")
    n_cuts = cut_pos.numel()
    if n_cuts > ctr_rank_resample_max_cuts():
        raise ValueError(f"{who}: {n_cuts} cuts: one call takes at most {ctr_rank_resample_max_cuts()}")
    W = RANK_RESAMPLE_WORDS + 2 * n_cuts

    def launch(m, ld, nu, R, out, ap):
        nws = lib.mvin_ctr_rank_resample_ws_bytes(n, R)
        if nws < 0:
            _lib.check(int(nws), "mvin_ctr_rank_resample_ws_bytes")
        ws = torch.empty((int(nws),), dtype=torch.uint8, device=dev)
        _lib.check(lib.mvin_ctr_rank_resample(_p(image), n, _p(m), ld, nu, R, _p(cut_pos) if n_cuts else None, n_cuts, max_groups,
                                              _p(ws), _p(out), _p(ap), _stream()), "mvin_ctr_rank_resample")

    if n_units is None:
        if mult is not None:
            raise ValueError(f"{who}: mult needs n_units")
        out = torch.empty((1, W), dtype=torch.int64, device=dev)
        ap = torch.empty((1,), dtype=torch.float64, device=dev)
        launch(None, 0, 0, 1, out, ap)
        return out, ap
    n_units = int(n_units)
    if not 0 <= n_units < 1 << 31:
        raise ValueError(f"n_units={n_units}: expected 0 <= n_units < 2^31")
    if mult is not None:
        if not isinstance(mult, torch.Tensor) or mult.device != dev or mult.dtype != I32 or mult.dim() != 2 or mult.shape[1] < n_units \
                or not mult.is_contiguous():
            raise ValueError(f"{who}: mult: expected a contiguous int32 [R, >= {n_units}] tensor on {dev}")
        R = mult.shape[0]
        out = torch.empty((R, W), dtype=torch.int64, device=dev)
        ap = torch.empty((R,), dtype=torch.float64, device=dev)
        if R:
            launch(mult, max(mult.shape[1], 1), n_units, R, out, ap)
        return out, ap
    n_rep, first = int(n_rep), int(first)
    if n_rep < 0 or first < 0:
        raise ValueError(f"n_rep={n_rep} first={first}: expected values >= 0")
    budget = RANK_RESAMPLE_MULT_BYTES if budget_bytes is None else int(budget_bytes)
    per_rep = 4 * max(n_units, 1) + int(lib.mvin_ctr_rank_resample_ws_bytes(n, 1))
    step = max(1, budget // per_rep)
    out = torch.empty((n_rep, W), dtype=torch.int64, device=dev)
    ap = torch.empty((n_rep,), dtype=torch.float64, device=dev)
    buf = torch.empty((min(step, n_rep), max(n_units, 1)), dtype=I32, device=dev) if n_rep else None
    for r0 in range(0, n_rep, step):
        R = min(step, n_rep - r0)
        m = buf[:R]
        resample_multiplicities(n_units, R, seed=seed, first=first + r0, out=m)
        launch(m, max(n_units, 1), n_units, R, out[r0:r0 + R], ap[r0:r0 + R])
    return out, ap


def rank_resample_stats(out, ap_sum):
    """Per replicate, in float64 on the host, from ctr_rank_resample's ``out`` [R, 12 + 2 n_cuts] and ``ap_sum`` [R]: a dict of
    arrays [R] -- ``ap`` = ap_sum / M, ``auc`` = u2 / (2 M N), per criterion of OPERATING_CRITERIA its value at the replicate's
    best cut (``f1_max``, ``acc_max``, ``youden_max``, by operating_point_metrics' conventions) and its position (``f1_pos``,
    ...), ``ok`` = the replicate has both classes and did not overflow (the rest is NaN where it is False) -- and ``cuts``: per
    fixed cut a dict of ``acc`` / ``f1`` / ``precision`` / ``recall`` arrays [R]."""
    o = np.asarray(out).astype(np.int64)
    s = np.asarray(ap_sum, dtype=np.float64).reshape(-1)
    if o.ndim != 2 or o.shape[1] < RANK_RESAMPLE_WORDS or (o.shape[1] - RANK_RESAMPLE_WORDS) % 2 or o.shape[0] != s.size:
        raise ValueError(f"expected out [R, 12 + 2 n_cuts] and ap_sum [R], got {o.shape} and {s.shape}")
    R, n_cuts = o.shape[0], (o.shape[1] - RANK_RESAMPLE_WORDS) // 2
    ok = (o[:, 0] > 0) & (o[:, 1] > 0) & (o[:, 2] >= 0) & np.isfinite(s)
    nan = np.full(R, np.nan)
    res = {"ok": ok, "ap": nan.copy(), "auc": nan.copy(), "cuts": [{k: nan.copy() for k in ("acc", "f1", "precision", "recall")}
                                                                   for _ in range(n_cuts)]}
    for name in OPERATING_CRITERIA:
        res[name + "_max"] = nan.copy()
        res[name + "_pos"] = np.full(R, -1, dtype=np.int64)
    for r in np.flatnonzero(ok):
        M, N = int(o[r, 0]), int(o[r, 1])
        res["ap"][r] = s[r] / np.float64(M)
        res["auc"][r] = np.float64(int(o[r, 2])) / (2.0 * np.float64(M) * np.float64(N))
        for c, name in enumerate(OPERATING_CRITERIA):
            tp, fp, pos = (int(v) for v in o[r, 3 + 3 * c:6 + 3 * c])
            res[name + "_max"][r] = operating_point_metrics(tp, fp, M, N)[name]
            res[name + "_pos"][r] = pos
        for k in range(n_cuts):
            met = operating_point_metrics(int(o[r, 12 + 2 * k]), int(o[r, 13 + 2 * k]), M, N)
            for key in ("acc", "f1", "precision", "recall"):
                res["cuts"][k][key][r] = met[key]
    return res


def percentile_interval(x, level):
    """se (ddof 1) and the percentile interval of the finite values of x: (se, lo, hi), NaN where undefined."""
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)]
    a = (1.0 - float(level)) / 2.0
    lo, hi = (float(np.quantile(x, a)), float(np.quantile(x, 1.0 - a))) if x.size else (float("nan"), float("nan"))
    return (float(np.std(x, ddof=1)) if x.size > 1 else float("nan")), lo, hi


def rank_resample_summary(out, ap_sum, level=0.95):
    """Intervals from ctr_rank_resample's replicates, on the host in float64 (rank_resample_stats per replicate): ``{"ap", "auc",
    "f1_max", "acc_max", "youden_max": {"se", "lo", "hi"}, "cuts": [{"acc", "f1", "precision", "recall": {"se", "lo", "hi"}}],
    "degenerate"}`` -- ``se`` the sample standard deviation (ddof 1) of the replicate values, ``lo`` / ``hi`` their percentiles
    at (1 - level) / 2 and 1 - (1 - level) / 2, ``degenerate`` the replicates left out because a class was empty (M == 0 or
    N == 0) or the weights overflowed."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level={level}: expected a value in (0, 1)")
    st = rank_resample_stats(out, ap_sum)

    def box(x):
        se, lo, hi = percentile_interval(x, level)
        return {"se": se, "lo": lo, "hi": hi}

    res = {k: box(st[k]) for k in ("ap", "auc") + tuple(c + "_max" for c in OPERATING_CRITERIA)}
    res["cuts"] = [{k: box(v) for k, v in cut.items()} for cut in st["cuts"]]
    res["degenerate"] = int((~st["ok"]).sum())
    return res


def paired_bootstrap_pvalue(d):
    """The two-sided bootstrap p-value of paired replicate differences ``d`` [R] (NaNs left out): ``min(1, 2 (1 + min(#{d <= 0},
    #{d >= 0})) / (R + 1))`` -- never 0.  NaN with no replicate."""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    d = d[np.isfinite(d)]
    if not d.size:
        return float("nan")
    return float(min(1.0, 2.0 * (1.0 + min((d <= 0).sum(), (d >= 0).sum())) / (d.size + 1.0)))


def placement_moments_max_models():
    """mvin_placement_moments_max_models: the models one mvin_placement_moments call takes (8)."""
    return int(_lib.load().mvin_placement_moments_max_models())


def placement_moments(place, labels, max_groups=0):
    """mvin_placement_moments: the exact sums and cross-products of K models' placements of the same rows.  ``place`` int64
    [K, n] (ctr_placements rows, dense, possibly strided between models), ``labels`` int32 [n].  A row is used when its label is
    0 / 1 and no model marked it -1.  Returns device tensors ``(cross int64 [2, K, K, 2], sums int64 [2, K], counts int64 [3])``:
    per class (0 negatives, 1 positives) the 96-bit sums of place[a] * place[b] as two unsigned 64-bit words (value = [0] + [1]
    * 2^32; each word is below 2^63, so its int64 reading is the word), the sums of place[a], and (used class 0, used class 1,
    bad).  ``max_groups``: 0 automatic, else a cap on the workgroups per model; it changes no bit.  Enqueues only."""
    lib = _lib.load()
    if not isinstance(place, torch.Tensor) or place.dim() != 2:
        raise ValueError("place: expected a [K, n] tensor")
    for t, name, dt in ((place, "place", torch.int64), (labels, "labels", I32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
        if t.dtype != dt:
            raise TypeError(f"{name}: expected {dt}, got {t.dtype}")
    K, n = place.shape
    if not 1 <= K <= placement_moments_max_models():
        raise ValueError(f"{K} models: mvin_placement_moments takes 1 .. {placement_moments_max_models()}")
    if labels.dim() != 1 or labels.numel() != n or not labels.is_contiguous():
        raise ValueError(f"labels {tuple(labels.shape)}: expected a contiguous [{n}] tensor")
    ld = place.stride(0) if K > 1 else max(n, 1)
    if n and ((n > 1 and place.stride(1) != 1) or ld < n):
        raise ValueError("place: rows must be dense (stride 1 along the rows of the split, models at least n apart)")
    max_groups = int(max_groups)
    if max_groups < 0 or n >= 1 << 31:
        raise ValueError(f"max_groups={max_groups} n={n}: expected max_groups >= 0 and n < 2^31")
    dev = place.device
    cross = torch.empty((2, K, K, 2), dtype=torch.int64, device=dev)
    sums = torch.empty((2, K), dtype=torch.int64, device=dev)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    _lib.check(lib.mvin_placement_moments(_p(place) if n else None, ld, K, _p(labels) if n else None, n, max_groups, _p(cross), _p(sums),
                                          _p(counts), _stream()), "mvin_placement_moments")
    return cross, sums, counts


def delong_from_moments(cross, sums, counts):
    """DeLong's AUCs and their covariance matrix from placement_moments' integers (host arrays [2, K, K, 2], [2, K], [3]), in
    exact arithmetic until the last step.  With m positives, n negatives, T_c[a, b] the 96-bit value and s_c[a] the sums:
      S10[a, b] = (m T_1 - s_1a s_1b) / (m (m - 1) 4 n^2),   S01[a, b] = (n T_0 - s_0a s_0b) / (n (n - 1) 4 m^2),
      cov[a, b] = S10 / m + S01 / n  -- a fractions.Fraction, rounded to float64 once;
      auc[a] = float64(s_1a) / (2.0 * float64(m) * float64(n)) -- ctr_metrics_from_counts' operations, so its bits.
    Returns ``{"auc": f64 [K], "cov": f64 [K, K], "n_pos": m, "n_neg": n}``.  The variance treats the rows as independent draws.
    ValueError when ``bad > 0`` (a row some model marked invalid) and when a class has fewer than two rows (the variance is
    undefined)."""
    from fractions import Fraction
    cr = np.asarray(cross)
    sm = np.asarray(sums)
    ct = np.asarray(counts).reshape(-1)
    if cr.ndim != 4 or cr.shape[0] != 2 or cr.shape[1] != cr.shape[2] or cr.shape[3] != 2 or sm.shape != (2, cr.shape[1]) or ct.size != 3:
        raise ValueError(f"expected cross [2, K, K, 2], sums [2, K] and counts [3], got {cr.shape}, {sm.shape}, {ct.shape}")
    K = cr.shape[1]
    n, m, bad = int(ct[0]), int(ct[1]), int(ct[2])
    if bad > 0:
        raise ValueError(f"{bad} row(s) with a non-finite score (a placement of -1)")
    if m < 2 or n < 2:
        raise ValueError(f"{m} positive and {n} negative rows: DeLong's variance needs at least two of each class")
    word = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF               # noqa: E731  (an unsigned word read as int64)
    T = [[[word(cr[c, a, b, 0]) + (word(cr[c, a, b, 1]) << 32) for b in range(K)] for a in range(K)] for c in range(2)]
    s = [[int(sm[c, a]) for a in range(K)] for c in range(2)]
    cov = np.empty((K, K), dtype=np.float64)
    for a in range(K):
        for b in range(K):
            s10 = Fraction(m * T[1][a][b] - s[1][a] * s[1][b], m * (m - 1) * 4 * n * n)
            s01 = Fraction(n * T[0][a][b] - s[0][a] * s[0][b], n * (n - 1) * 4 * m * m)
            f = s10 / m + s01 / n
            cov[a, b] = f.numerator / f.denominator            # int / int: correctly rounded
    auc = np.array([np.float64(s[1][a]) / (2.0 * np.float64(m) * np.float64(n)) for a in range(K)], dtype=np.float64)
    return {"auc": auc, "cov": cov, "n_pos": m, "n_neg": n}


def delong_interval(auc, var, level=0.95):
    """The Wald interval of an AUC from its DeLong variance: ``(se, lo, hi)`` with se = sqrt(var) and auc -+ z se clipped to
    [0, 1], z the normal quantile of 1 - (1 - level) / 2 (statistics.NormalDist)."""
    import math
    from statistics import NormalDist
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"level={level}: expected a value in (0, 1)")
    se = math.sqrt(max(float(var), 0.0))
    z = NormalDist().inv_cdf(1.0 - (1.0 - level) / 2.0)
    return se, max(0.0, float(auc) - z * se), min(1.0, float(auc) + z * se)


def delong_test(auc, cov, a, b):
    """DeLong's paired test of ``auc[a] - auc[b]`` for two models scored on the same rows: ``{"diff", "se", "z", "p"}`` with
    var = cov[a, a] + cov[b, b] - 2 cov[a, b] clamped at 0, z = diff / se and the two-sided p = erfc(|z| / sqrt 2).  With
    var == 0: z = 0 and p = 1 when diff == 0, else z = +-inf and p = 0."""
    import math
    auc, cov = np.asarray(auc, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    diff = float(auc[a] - auc[b])
    var = max(float(cov[a, a] + cov[b, b] - 2.0 * cov[a, b]), 0.0)
    se = math.sqrt(var)
    if se == 0.0:
        z = 0.0 if diff == 0.0 else math.copysign(math.inf, diff)
        p = 1.0 if diff == 0.0 else 0.0
    else:
        z = diff / se
        p = math.erfc(abs(z) / math.sqrt(2.0))
    return {"diff": diff, "se": se, "z": z, "p": p}


def cluster_csr(ids, order_dtype=np.int32):
    """The stable grouping of rows by an integer id on the host: ``(order int32 [n], seg_ptr int64 [I + 1], cluster_ids [I])`` with
    ``ids[order]`` ascending, equal ids in row order, and cluster i = positions ``seg_ptr[i]:seg_ptr[i+1]`` of ``order`` -- what
    placement_cluster_moments, segment_sums and (as user segments) ctr_counts_segments take.  ``ids``: a one-dimensional integer
    array of fewer than 2^31 rows; anything else raises ValueError.  ``order_dtype``: np.int64 for an order index_select takes."""
    ids = np.asarray(ids)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError(f"cluster ids: expected a one-dimensional integer array, got {ids.dtype} {ids.shape}")
    n = ids.size
    if n >= 1 << 31:
        raise ValueError(f"n={n}: expected fewer than 2^31 rows")
    if n == 0:
        return np.zeros(0, order_dtype), np.zeros(1, np.int64), ids[:0].copy()
    lo, hi = int(ids.min()), int(ids.max())
    if hi - lo < (1 << 31):                                     # the stable argsort as ONE sort of (id, row) keys
        order = np.sort((ids.astype(np.int64, copy=False) - lo) * n + np.arange(n, dtype=np.int64)) % n
    else:
        order = np.argsort(ids, kind="stable")
    s = ids[order]
    first = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    seg_ptr = np.concatenate((first, [n])).astype(np.int64)
    return order.astype(order_dtype, copy=False), seg_ptr, s[first]


def _cluster_grouping(seg_ptr, order, n, name):
    """What placement_cluster_moments and segment_sums check alike: seg_ptr int64 [I + 1] and order int32 [n] or None."""
    _chk(seg_ptr, torch.int64, "seg_ptr")
    if seg_ptr is None or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
        raise ValueError(f"{name}: seg_ptr: expected a contiguous int64 [I + 1] tensor")
    if order is not None:
        _chk(order, I32, "order")
        if order.dim() != 1 or order.numel() != n:
            raise ValueError(f"{name}: order {tuple(order.shape)}: expected a contiguous int32 [{n}] tensor or None")
    I = seg_ptr.numel() - 1
    if I >= 1 << 31 or n >= 1 << 31:
        raise ValueError(f"{name}: n={n} clusters={I}: expected fewer than 2^31 of each")
    return I


def placement_cluster_moments(place, labels, seg_ptr, order=None, max_groups=0, out=None):
    """mvin_placement_cluster_moments: per-cluster sums of K models' placements and their Gram matrix, exact.  ``place`` int64
    [K, n] and ``labels`` int32 [n] as placement_moments takes them (and a row is used under its rule); ``seg_ptr`` int64
    [I + 1] and ``order`` int32 [n] or None group the rows (cluster_csr; a malformed grouping is clamped, include/mvin_hip.h).
    Returns device tensors ``(csum int64 [I, 2 + 2K], gram int64 [K + 2, K + 2, 2, 4], totals int64 [4 + 2K])``: per cluster
    (m_i, n_i, A_i^1..K, B_i^1..K); the limb sums of G = sum_i z_i z_i^T, z_i = (m_i, n_i, A_i - B_i) (each word below 2^63, so
    its int64 reading is the word; clustered_delong_from_gram joins them); and (I with a used row, m, n, s1^1..K, s0^1..K, bad).
    ``max_groups``: 0 automatic, else a cap on the workgroups per launch; it changes no bit.  ``out``: the same three to write
    into.  Enqueues only."""
    lib = _lib.load()
    if not isinstance(place, torch.Tensor) or place.dim() != 2:
        raise ValueError("place: expected a [K, n] tensor")
    for t, name, dt in ((place, "place", torch.int64), (labels, "labels", I32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
        if t.dtype != dt:
            raise TypeError(f"{name}: expected {dt}, got {t.dtype}")
    K, n = place.shape
    if not 1 <= K <= placement_moments_max_models():
        raise ValueError(f"{K} models: mvin_placement_cluster_moments takes 1 .. {placement_moments_max_models()}")
    if labels.dim() != 1 or labels.numel() != n or not labels.is_contiguous():
        raise ValueError(f"labels {tuple(labels.shape)}: expected a contiguous [{n}] tensor")
    ld = place.stride(0) if K > 1 else max(n, 1)
    if n and ((n > 1 and place.stride(1) != 1) or ld < n):
        raise ValueError("place: rows must be dense (stride 1 along the rows of the split, models at least n apart)")
    max_groups = int(max_groups)
    if max_groups < 0:
        raise ValueError(f"max_groups={max_groups}: expected a value >= 0")
    I = _cluster_grouping(seg_ptr, order, n, "placement_cluster_moments")
    dev = place.device
    if out is None:
        out = (torch.empty((I, 2 + 2 * K), dtype=torch.int64, device=dev), torch.empty((K + 2, K + 2, 2, 4), dtype=torch.int64, device=dev),
               torch.empty((4 + 2 * K,), dtype=torch.int64, device=dev))
    if len(out) != 3:
        raise ValueError("out: expected (csum, gram, totals)")
    csum, gram, totals = (_chk(t, torch.int64, "out " + name) for t, name in zip(out, ("csum", "gram", "totals")))
    if (csum is None or gram is None or totals is None or tuple(csum.shape) != (I, 2 + 2 * K) or tuple(gram.shape) != (K + 2, K + 2, 2, 4)
            or tuple(totals.shape) != (4 + 2 * K,)):
        raise ValueError(f"out: expected int64 csum [{I}, {2 + 2 * K}], gram [{K + 2}, {K + 2}, 2, 4] and totals [{4 + 2 * K}]")
    _lib.check(lib.mvin_placement_cluster_moments(_p(place) if n else None, ld, K, _p(labels) if n else None, n, _p(order) if n else None,
                                                  _p(seg_ptr), I, max_groups, _p(csum) if I else None, _p(gram), _p(totals), _stream()),
               "mvin_placement_cluster_moments")
    return csum, gram, totals


def clustered_delong_from_gram(gram, totals):
    """The AUCs and their cluster-robust covariance matrix (Obuchowski 1997) from placement_cluster_moments' integers (host arrays
    [K + 2, K + 2, 2, 4] and [4 + 2K]), in exact arithmetic until the last step.  With I clusters, m positives, n negatives,
    G the joined Gram matrix and c_a = (-n s1^a, m s0^a, m n unit_a):
      sum_i e_i^a e_i^b = c_a^T G c_b,   cov[a, b] = I c_a^T G c_b / ((I - 1) 4 m^4 n^4)  -- a Fraction, rounded to float64 once;
      auc[a] = float64(s1^a) / (2.0 * float64(m) * float64(n)) -- ctr_metrics_from_counts' operations, so its bits.
    e_i^a = m n D_i^a - n m_i s1^a + m n_i s0^a is cluster i's share of model a's AUC deviation (sum_i e_i = 0): the cluster, not
    the row, is the unit.  Returns ``{"auc", "cov", "n_pos", "n_neg", "n_clusters"}``.  ValueError when ``bad > 0``, when a class
    has no row, and with fewer than two clusters."""
    from fractions import Fraction
    g = np.asarray(gram)
    t = np.asarray(totals).reshape(-1)
    if g.ndim != 4 or g.shape[0] != g.shape[1] or g.shape[0] < 3 or g.shape[2:] != (2, 4) or t.size != 2 * g.shape[0]:
        raise ValueError(f"expected gram [K + 2, K + 2, 2, 4] and totals [4 + 2K], got {g.shape} and {t.shape}")
    K = g.shape[0] - 2
    I, m, n, bad = int(t[0]), int(t[1]), int(t[2]), int(t[3 + 2 * K])
    if bad > 0:
        raise ValueError(f"{bad} row(s) with a non-finite score (a placement of -1)")
    if m < 1 or n < 1:
        raise ValueError(f"{m} positive and {n} negative rows: the AUC needs a row of each class")
    if I < 2:
        raise ValueError(f"{I} cluster(s) with a used row: the clustered variance needs at least two")
    word = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF               # noqa: E731  (an unsigned word read as int64)
    G = [[sum((word(g[p, q, 0, k]) - word(g[p, q, 1, k])) << (32 * k) for k in range(4)) for q in range(K + 2)] for p in range(K + 2)]
    s1 = [int(v) for v in t[3:3 + K]]
    s0 = [int(v) for v in t[3 + K:3 + 2 * K]]
    c = [[-n * s1[a], m * s0[a]] + [m * n if b == a else 0 for b in range(K)] for a in range(K)]
    Gc = [[sum(G[p][q] * c[b][q] for q in range(K + 2)) for p in range(K + 2)] for b in range(K)]
    den = (I - 1) * 4 * m ** 4 * n ** 4
    cov = np.empty((K, K), dtype=np.float64)
    for a in range(K):
        for b in range(K):
            f = Fraction(I * sum(c[a][p] * Gc[b][p] for p in range(K + 2)), den)
            cov[a, b] = f.numerator / f.denominator            # int / int: correctly rounded
    auc = np.array([np.float64(s1[a]) / (2.0 * np.float64(m) * np.float64(n)) for a in range(K)], dtype=np.float64)
    return {"auc": auc, "cov": cov, "n_pos": m, "n_neg": n, "n_clusters": I}


def segment_sums_max_cols():
    """mvin_segment_sums_max_cols: the columns one mvin_segment_sums_f64 call takes (1024)."""
    return int(_lib.load().mvin_segment_sums_max_cols())


def segment_sums(vals, seg_ptr, order=None, out=None):
    """mvin_segment_sums_f64: per-cluster column sums of ``vals`` (f64 [n, M] on the device, dense rows that may be strided) for
    the grouping ``seg_ptr`` int64 [I + 1] / ``order`` int32 [n] or None (cluster_csr).  Returns f64 [I, M].  One fixed summation
    order per cell (include/mvin_hip.h: 64 interleaved partial sums in row order, folded 32 .. 1), so a cell's bits depend on its
    cluster's rows and its column only; an empty cluster gives +0.0; NaN and infinities propagate.  A table wider than
    segment_sums_max_cols() goes through one launch per block of columns, which changes no bit.  ``out``: f64 [I, M] to write into.
    Enqueues only."""
    lib = _lib.load()
    if not isinstance(vals, torch.Tensor) or vals.dim() != 2:
        raise ValueError("vals: expected a [n, M] tensor")
    if vals.dtype != torch.float64:
        raise TypeError(f"vals: expected torch.float64, got {vals.dtype}")
    if not vals.is_cuda:
        raise _lib.MvinHipError("vals: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    n, M = vals.shape
    ld = vals.stride(0) if n > 1 else max(M, 1)
    if n and ((M > 1 and vals.stride(1) != 1) or ld < M):
        raise ValueError("vals: rows must be dense (stride 1 along the columns, rows at least M doubles apart)")
    I = _cluster_grouping(seg_ptr, order, n, "segment_sums")
    cap = segment_sums_max_cols()
    if out is None:
        out = torch.empty((I, M), dtype=torch.float64, device=vals.device)
    if _chk(out, torch.float64, "out") is None or tuple(out.shape) != (I, M):
        raise ValueError(f"out: expected f64 [{I}, {M}]")
    if I == 0 or M == 0:
        return out

    def launch(c0, w, dst):
        _lib.check(lib.mvin_segment_sums_f64(_p(vals, c0) if n else None, n, w, ld, _p(order) if n else None, _p(seg_ptr), I, _p(dst),
                                             _stream()), "mvin_segment_sums_f64")

    if M <= cap:
        launch(0, M, out)
        return out
    for c0 in range(0, M, cap):
        w = min(cap, M - c0)
        part = torch.empty((I, w), dtype=torch.float64, device=vals.device)
        launch(c0, w, part)
        out[:, c0:c0 + w].copy_(part)
    return out


CTR_CALIB_MAX_BINS = 64      # MVIN_CTR_CALIB_MAX_BINS
CTR_CALIB_SUMS = ("loss", "r2", "r", "rz", "w", "wz", "wz2", "p")
CTR_MASS_ONE = float(1 << 40)          # the confidence mass of p = 1 (mvin_ctr_calib: floor(p * 2^40) per pair)


def calib_edges(n_bins, a=1.0, b=0.0):
    """The z-space edges of ``n_bins`` uniform probability bins under the map ``p = sigmoid(a z + b)``: a float32 numpy array
    [n_bins - 1], edge k = (logit(k / n_bins) - b) / a computed in float64 and rounded to float32 (mvin_ctr_calib bins the f32
    logit itself against them).  ``a <= 0`` raises ValueError: the map must be increasing."""
    import numpy as np
    n_bins, a, b = int(n_bins), float(a), float(b)
    if not 1 <= n_bins <= CTR_CALIB_MAX_BINS:
        raise ValueError(f"n_bins={n_bins}: expected 1 .. {CTR_CALIB_MAX_BINS}")
    if not (a > 0.0 and np.isfinite(a) and np.isfinite(b)):
        raise ValueError(f"calibration map a={a}, b={b}: expected a finite map with a > 0")
    q = np.arange(1, n_bins, dtype=np.float64) / n_bins
    return ((np.log(q) - np.log1p(-q) - b) / a).astype(np.float32)


def ctr_calib(logits, labels, seg_len, a=1.0, b=0.0, targets=(0.0, 1.0), edges=None, max_groups=0):
    """mvin_ctr_calib: calibration sums and reliability bins of every segment under ``p = sigmoid(a z + b)``.  ``logits`` f32 and
    ``labels`` int32 as ctr_counts takes them (1-D of S * seg_len pairs, or [S, seg_len] with dense rows).  ``targets`` =
    (y0, y1), the regression targets of label 0 / 1 ((0, 1), or Platt's smoothed ones).  ``edges``: ascending f32 z-edges
    (calib_edges; a device tensor, a host array or None = one bin).  Returns ``(sums f64 [S, 8] (CTR_CALIB_SUMS), counts int64
    [S, 2] (valid, bad), bins int64 [S, n_bins, 3] (count, positives, confidence mass))`` on the device.  Enqueues only when
    ``edges`` is a device tensor or None; the sums are the same bits for every ``max_groups``.  LIMIT: the confidence mass is an
    int64 sum of values up to 2^40, exact while a bin holds fewer than 2^23 pairs."""
    import numpy as np
    lib = _lib.load()
    seg_len = int(seg_len)
    if seg_len < 1:
        raise ValueError(f"seg_len={seg_len}: expected >= 1")
    if isinstance(logits, torch.Tensor) and logits.dim() == 1:
        if logits.numel() % seg_len:
            raise ValueError(f"logits: {logits.numel()} pairs are not whole segments of {seg_len}")
        _chk(logits, F32, "logits")
        logits = logits.view(-1, seg_len)
    if isinstance(labels, torch.Tensor) and labels.dim() == 1:
        _chk(labels, I32, "labels")
        labels = labels.view(-1, seg_len) if labels.numel() % seg_len == 0 else labels
    _ctr_rows(logits, "logits", F32)
    _ctr_rows(labels, "labels", I32)
    if tuple(logits.shape) != tuple(labels.shape) or logits.shape[1] != seg_len:
        raise ValueError(f"logits {tuple(logits.shape)} and labels {tuple(labels.shape)}: expected [S, {seg_len}] both")
    S = logits.shape[0]
    ld = logits.stride(0) if S > 1 else seg_len
    if S > 1 and labels.stride(0) != ld:
        raise ValueError(f"labels: row stride {labels.stride(0)}, logits: {ld}; the two must share one layout")
    dev = logits.device
    if edges is None:
        edges = torch.empty((0,), dtype=F32, device=dev)
    elif not isinstance(edges, torch.Tensor):
        e = np.ascontiguousarray(edges, dtype=np.float32)
        if e.ndim != 1 or (e.size > 1 and not (np.diff(e) >= 0).all()) or np.isnan(e).any():
            raise ValueError("edges: expected an ascending 1-D array without NaN")
        edges = torch.from_numpy(e).to(dev)
    _chk(edges, F32, "edges")
    if edges.dim() != 1 or edges.numel() + 1 > CTR_CALIB_MAX_BINS:
        raise ValueError(f"edges: expected [n_bins - 1] with n_bins <= {CTR_CALIB_MAX_BINS}")
    n_bins = edges.numel() + 1
    y0, y1 = (float(t) for t in targets)
    sums = torch.empty((S, 8), dtype=torch.float64, device=dev)
    counts = torch.empty((S, 2), dtype=torch.int64, device=dev)
    bins = torch.empty((S, n_bins, 3), dtype=torch.int64, device=dev)
    if S == 0:
        return sums, counts, bins
    nws = lib.mvin_ctr_calib_ws_bytes(S, seg_len)
    if nws < 0:
        _lib.check(int(nws), "mvin_ctr_calib_ws_bytes")
    ws = torch.empty(((nws + 7) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.mvin_ctr_calib(_p(logits), _p(labels), S, seg_len, ld, float(a), float(b), y0, y1,
                                  _p(edges) if n_bins > 1 else None, n_bins, int(max_groups), _p(ws), _p(sums), _p(counts),
                                  _p(bins), _stream()), "mvin_ctr_calib")
    return sums, counts, bins


def ctr_calibration_from_sums(sums, counts, bins):
    """The calibration report of every segment from ctr_calib's three results copied to the host ([S, 8] / [S, 2] /
    [S, n_bins, 3], or one segment's rows), in float64.  Returns a dict of arrays over the segments: ``logloss`` = sum l / n,
    ``brier`` = sum r^2 / n, ``mean_pred``, ``base_rate``, ``ne`` = logloss over the entropy of the base rate (NaN with one
    class), ``ece`` = sum_k (c_k / n) |pos_k / c_k - conf_k / c_k|, ``mce`` = the largest such gap over the non-empty bins,
    ``n``, and per bin ``bin_count``, ``bin_rate`` and ``bin_conf`` (NaN in empty bins).  A segment with ``bad > 0`` raises
    ValueError, as ctr_metrics_from_counts does."""
    import numpy as np
    s = np.asarray(sums, dtype=np.float64)
    c = np.asarray(counts).astype(np.int64, copy=False)
    k = np.asarray(bins).astype(np.int64, copy=False)
    if s.ndim == 1:
        s, c, k = s.reshape(1, -1), c.reshape(1, -1), k.reshape((1,) + k.shape)
    if s.ndim != 2 or s.shape[1] != 8 or c.shape != (s.shape[0], 2) or k.ndim != 3 or k.shape[0] != s.shape[0] or k.shape[2] != 3:
        raise ValueError(f"expected sums [S, 8], counts [S, 2], bins [S, n_bins, 3]; got {s.shape}, {c.shape}, {k.shape}")
    bad = c[:, 1]
    if (bad > 0).any():
        i = int(np.flatnonzero(bad > 0)[0])
        raise ValueError(f"segment {i}: {int(bad[i])} non-finite logit(s) or label(s) other than 0 / 1")
    n = c[:, 0].astype(np.float64)
    cnt = k[:, :, 0].astype(np.float64)
    pos = k[:, :, 1].astype(np.float64)
    conf = k[:, :, 2].astype(np.float64) / CTR_MASS_ONE
    with np.errstate(divide="ignore", invalid="ignore"):
        logloss = s[:, 0] / n
        brier = s[:, 1] / n
        mean_pred = s[:, 7] / n
        base = pos.sum(axis=1) / n
        h = -(base * np.log(base) + (1.0 - base) * np.log1p(-base))
        ne = np.where((base > 0) & (base < 1), logloss / h, np.nan)
        rate = np.where(cnt > 0, pos / cnt, np.nan)
        mconf = np.where(cnt > 0, conf / cnt, np.nan)
        gap = np.where(cnt > 0, np.abs(rate - mconf), 0.0)
        ece = (cnt / n[:, None] * gap).sum(axis=1)
        mce = np.where(n > 0, gap.max(axis=1), np.nan)
        ece = np.where(n > 0, ece, np.nan)
    return dict(logloss=logloss, brier=brier, mean_pred=mean_pred, base_rate=base, ne=ne, ece=ece, mce=mce, n=c[:, 0].copy(),
                bin_count=k[:, :, 0].copy(), bin_rate=rate, bin_conf=mconf)


def platt_step(sums, n):
    """One damped Newton direction of the Platt fit from one segment's ctr_calib sums (a host row of 8) over ``n`` valid pairs.
    With the loss L(a, b) = sum l / n: gradient g = (sum r z, sum r) / n, Hessian H = [[sum w z^2, sum w z], [sum w z, sum w]] /
    n.  Returns ``(da, db, slope)``: the direction -H^-1 g and its slope g . d < 0; a Hessian that is singular (det H <= 1e-12
    H_aa H_bb) or indefinite, or a direction that does not descend, falls back to -g.  A pure host function."""
    import numpy as np
    s = np.asarray(sums, dtype=np.float64).reshape(-1)
    if s.size != 8 or n <= 0:
        raise ValueError("platt_step: expected one row of 8 sums and n > 0")
    n = float(n)
    ga, gb = s[3] / n, s[2] / n
    haa, hab, hbb = s[6] / n, s[5] / n, s[4] / n
    det = haa * hbb - hab * hab
    da, db = -ga, -gb
    if np.isfinite(det) and haa > 0.0 and hbb > 0.0 and det > 1e-12 * haa * hbb:
        na, nb = -(hbb * ga - hab * gb) / det, -(haa * gb - hab * ga) / det
        if np.isfinite(na) and np.isfinite(nb) and ga * na + gb * nb < 0.0:
            da, db = na, nb
    return float(da), float(db), float(ga * da + gb * db)


def ctr_counts_segments(scores, labels, seg_ptr, threshold=0.5, max_len=None, form=0, out=None):
    """mvin_ctr_counts_segments: ctr_counts' six integers (int64 [n_seg, 6], ``CTR_COLUMNS``) for the segments
    ``scores[seg_ptr[s]:seg_ptr[s+1]]`` of a flat f32 buffer with int32 ``labels`` -- the rows of every user of a split, for
    per-user AUC (gauc_from_counts).  tp / fp count ``score >= threshold`` (0.5 for sigmoid scores, 0 for logits).
    ``max_len`` and ``form`` are rank_segments' (``max_len=None`` reads the bound from ``seg_ptr``: ONE synchronisation); LIMIT:
    ``max_len`` <= CTR_SEG_CAP.  Returns ``(counts, status int64 [2])`` (``out``: the same two; status is accumulated): a segment
    longer than ``max_len`` or with pointers out of order is a row of -1 and is counted in status[0]."""
    lib = _lib.load()
    scores, seg_ptr, n_seg, _, _, _, max_len, form = _segments_common(scores, seg_ptr, None, None, max_len, form,
                                                                      "ctr_counts_segments")
    _chk(labels, I32, "labels")
    if labels is None or labels.dim() != 1 or labels.numel() != scores.numel():
        raise ValueError(f"labels: expected int32 [{scores.numel()}]")
    if max_len > CTR_SEG_CAP:
        raise ValueError(f"max_len={max_len}: mvin_ctr_counts_segments takes segments of at most {CTR_SEG_CAP} entries")
    dev = scores.device
    if out is None:
        out = (torch.empty((n_seg, 6), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
    counts, status = out
    _chk(counts, torch.int64, "out counts")
    _chk(status, torch.int64, "out status")
    if tuple(counts.shape) != (n_seg, 6) or status.numel() != 2:
        raise ValueError(f"out: expected counts [{n_seg}, 6] and status [2]")
    T = scores.numel()
    anyp = _p(seg_ptr)                          # an empty array: any valid pointer, nothing is read or written through it
    _lib.check(lib.mvin_ctr_counts_segments(_p(scores) if T else None, _p(labels) if T else None, T, _p(seg_ptr), n_seg,
                                            float(threshold), max_len, form, _p(counts) if n_seg else anyp, _p(status), _stream()),
               "mvin_ctr_counts_segments")
    return counts, status


def gauc_from_counts(counts):
    """GAUC from ctr_counts_segments rows (a host array [U, 6], one row per user): a dict of ``weighted`` -- the
    impression-weighted mean of the users' AUCs, w_u = n_pos + n_neg -- ``mean`` (unweighted), ``users`` (those with both
    classes, the only ones averaged) and ``skipped_users`` (one class or no rows).  Both means are NaN without such a user.  A
    row with ``bad > 0`` or a padding row (-1) raises ValueError."""
    import numpy as np
    c = np.asarray(counts)
    if c.ndim == 1:
        c = c.reshape(1, -1)
    if c.ndim != 2 or c.shape[1] != 6:
        raise ValueError(f"counts: expected [U, 6], got {c.shape}")
    c = c.astype(np.int64, copy=False)
    if (c[:, 5] != 0).any():
        u = int(np.flatnonzero(c[:, 5] != 0)[0])
        raise ValueError(f"segment {u}: " + ("not counted (longer than max_len, or pointers out of order)" if c[u, 5] < 0 else
                                             f"{int(c[u, 5])} non-finite score(s) or label(s) other than 0 / 1"))
    n_pos, n_neg, u2 = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64), c[:, 4].astype(np.float64)
    both = (c[:, 0] > 0) & (c[:, 1] > 0)
    users = int(both.sum())
    if users == 0:
        return dict(weighted=float("nan"), mean=float("nan"), users=0, skipped_users=int(c.shape[0]))
    auc = u2[both] / (2.0 * n_pos[both] * n_neg[both])
    w = n_pos[both] + n_neg[both]
    return dict(weighted=float((w * auc).sum() / w.sum()), mean=float(auc.mean()), users=users,
                skipped_users=int(c.shape[0]) - users)


def _kg_index(index, seeds):
    eptr, edst, erel = index
    _chk(eptr, torch.int64, "eptr")
    _chk(edst, I32, "edst")
    _chk(erel, I32, "erel")
    _chk(seeds, I32, "seeds")
    if eptr.dim() != 1 or eptr.numel() < 1 or edst.dim() != 1 or tuple(erel.shape) != tuple(edst.shape) or seeds.dim() != 1:
        raise ValueError("edge index: expected (eptr int64 [nE+1], edst int32 [M], erel int32 [M]) and seeds int32 [n]")
    return eptr, edst, erel, eptr.numel() - 1, edst.numel()


def _kg_ws(lib, n_entity, M, dev):
    nws = lib.mvin_kg_explore_ws_bytes(n_entity, M)
    if nws < 0:
        _lib.check(int(nws), "mvin_kg_explore_ws_bytes")
    return torch.empty(((nws + 7) // 8,), dtype=torch.int64, device=dev) if nws > 0 else None


def kg_field(index, seeds, hops):
    """mvin_kg_field: the KG edges within ``hops`` levels of ``seeds`` (int32 ids on the device; repeats and ids out of range
    are fine).  ``index``: a data_prep.kg_edge_index triple.  Returns ``(field_bits int32 [ceil(M/32)], counts int64 [hops+1])``
    on the device: bit e of the bitmap (word e // 32, bit e % 32) is edge slot e; counts = |F_1| .. |F_hops|, then the number of
    field edges.  Enqueues only: no synchronisation, no copy to the host."""
    lib = _lib.load()
    eptr, edst, erel, nE, M = _kg_index(index, seeds)
    dev = eptr.device
    bits = torch.empty(((M + 31) // 32,), dtype=I32, device=dev)
    counts = torch.empty((int(hops) + 1 if 1 <= int(hops) <= 8 else 1,), dtype=torch.int64, device=dev)
    ws = _kg_ws(lib, nE, M, dev) if M else None
    _lib.check(lib.mvin_kg_field(_p(eptr), _p(edst) if M else None, _p(erel) if M else None, nE, M,
                                 _p(seeds) if seeds.numel() else None, seeds.numel(), int(hops), _p(ws),
                                 _p(bits) if M else None, _p(counts), _stream()), "mvin_kg_field")
    return bits, counts


def kg_explore(index, adj_entity, adj_relation, seeds, hops, explored_bits, out=None):
    """mvin_kg_explore: the KG edges the adjacency ``(adj_entity, adj_relation)`` (int32 [nE, K] on the device) reaches within
    ``hops`` levels of ``seeds``; a slot that is no edge of ``index`` is ignored and not followed.  ``explored_bits`` (int32
    [ceil(M/32)], zeros to begin with) is OR-updated in place, so feeding one adjacency after another accumulates.  Returns
    counts int64 [3] on the device (``out`` if given): edges this adjacency explores, edges newly set, edges set now.
    Enqueues only."""
    lib = _lib.load()
    eptr, edst, erel, nE, M = _kg_index(index, seeds)
    dev = eptr.device
    _chk(adj_entity, I32, "adj_entity")
    _chk(adj_relation, I32, "adj_relation")
    if adj_entity.dim() != 2 or adj_entity.shape[0] != nE or tuple(adj_relation.shape) != tuple(adj_entity.shape):
        raise ValueError(f"adj_entity / adj_relation: expected [{nE}, K] both")
    K = adj_entity.shape[1]
    _chk(explored_bits, I32, "explored_bits")
    if tuple(explored_bits.shape) != ((M + 31) // 32,):
        raise ValueError(f"explored_bits: expected [{(M + 31) // 32}]")
    if out is None:
        out = torch.empty((3,), dtype=torch.int64, device=dev)
    _chk(out, torch.int64, "out")
    if tuple(out.shape) != (3,):
        raise ValueError("out: expected [3]")
    if nE == 0:
        out.zero_()
        return out
    ws = _kg_ws(lib, nE, M, dev) if M else None
    _lib.check(lib.mvin_kg_explore(_p(eptr), _p(edst) if M else None, _p(erel) if M else None, nE, M, _p(adj_entity),
                                   _p(adj_relation), K, _p(seeds) if seeds.numel() else None, seeds.numel(), int(hops), _p(ws),
                                   _p(explored_bits) if M else None, _p(out), _stream()), "mvin_kg_explore")
    return out


RANK_METRICS = ("precision", "recall", "hit_ratio", "mrr", "map", "ndcg", "ndcg_ideal")
RANK_MISSING = 0x7FC00000    # the bits mvin_rank_positives writes as the value of an entry that no eligible column carries


def _rank_csr(pair, rows, name):
    ptr, ids = pair
    _chk(ptr, torch.int64, f"{name} ptr")
    _chk(ids, I32, f"{name} ids")
    if ptr.dim() != 1 or ptr.numel() != rows + 1:
        raise ValueError(f"{name} ptr: {ptr.numel()} entries for {rows} rows")
    if ids.dim() != 1:
        raise ValueError(f"{name} ids: expected a 1-D tensor")
    return ptr, ids


def rank_positives(scores, pos, cand_ids=None, col_offset=0, excl=None, out=None):
    """mvin_rank_positives: where the named items of every row land in the row's ranking, without ranking it.  ``scores``,
    ``cand_ids``, ``col_offset`` and ``excl`` are topk_rows's ([rows, n] f32 with dense rows, rows may be strided; item id per
    column; ``(ptr, ids)`` CSR of excluded ids per row, ascending).  ``pos``: a ``(ptr int64 [rows+1], ids int32 [T])`` CSR of the
    items to rank per row, each row ascending and distinct; ``ptr`` holds offsets into ``ids`` AND into the outputs, so a slice
    ``ptr[r0:r1+1]`` with the whole ``ids`` ranks rows r0 .. r1 into their places of whole-size outputs.  Returns
    ``(counts int32 [T, 3], vals f32 [T], eligible int32 [rows])`` (``out``: the same triple to write into): per entry
    (greater, equal_before, equal_after) among the row's eligible columns and the input bits of its score -- (-1, -1, -1) and a
    quiet NaN when no eligible column carries the id -- and per row the number of eligible columns.  greater + equal_before is the
    item's index in topk_rows's output.  Enqueues only: no synchronisation, no copy to the host."""
    lib = _lib.load()
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise _lib.MvinHipError("scores: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if scores.dtype != F32:
        raise TypeError(f"scores: expected {F32}, got {scores.dtype}")
    if scores.dim() != 2 or (scores.shape[1] > 1 and scores.stride(1) != 1) or scores.stride(0) < scores.shape[1]:
        raise ValueError("scores: expected a [rows, n] tensor with dense rows")
    rows, n = scores.shape
    dev = scores.device
    if cand_ids is not None:
        _chk(cand_ids, I32, "cand_ids")
        if cand_ids.numel() != n:
            raise ValueError(f"cand_ids: {cand_ids.numel()} ids for {n} columns")
    if pos is None or len(pos) != 2:
        raise ValueError("pos: expected a (ptr, ids) pair")
    pptr, pids = _rank_csr(pos, rows, "pos")
    T = pids.numel()
    eptr = eids = None
    if excl is not None:
        eptr, eids = _rank_csr(excl, rows, "excl")
    if out is None:
        out = (torch.empty((T, 3), dtype=I32, device=dev), torch.empty((T,), dtype=F32, device=dev),
               torch.empty((rows,), dtype=I32, device=dev))
    counts, vals, eligible = out
    _chk(counts, I32, "out counts")
    _chk(vals, F32, "out vals")
    _chk(eligible, I32, "out eligible")
    if tuple(counts.shape) != (T, 3) or tuple(vals.shape) != (T,) or tuple(eligible.shape) != (rows,):
        raise ValueError(f"out: expected counts [{T}, 3], vals [{T}] and eligible [{rows}]")
    if rows == 0:
        return counts, vals, eligible
    nws = lib.mvin_rank_positives_ws_bytes(rows, n, T)
    if nws < 0:
        _lib.check(int(nws), "mvin_rank_positives_ws_bytes")
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    ld = scores.stride(0) if rows > 1 else n
    anyp = _p(pptr)                             # an empty id array: any valid pointer, nothing is read or written through it
    _lib.check(lib.mvin_rank_positives(_p(scores) if n > 0 else None, rows, n, ld, _p(cand_ids), int(col_offset), _p(eptr),
                                       None if eptr is None else (_p(eids) if eids.numel() else _p(eptr)),
                                       _p(pptr), _p(pids) if T else anyp, _p(ws), _p(counts) if T else anyp,
                                       _p(vals) if T else anyp, _p(eligible), _stream()), "mvin_rank_positives")
    return counts, vals, eligible


def segments_wave_cap():
    """mvin_segments_wave_cap: the longest segment the wave form of topk_segments / rank_segments takes."""
    return int(_lib.load().mvin_segments_wave_cap())


def _segments_common(scores, seg_ptr, ids, excl, max_len, form, name):
    """The arguments topk_segments and rank_segments share, checked: (scores [T], seg_ptr, n_seg, ids, excl ptr, excl ids
    pointer, max_len, form)."""
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise _lib.MvinHipError("scores: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    _chk(scores, F32, "scores")
    if scores.dim() != 1:
        raise ValueError("scores: expected a flat [T] tensor")
    _chk(seg_ptr, torch.int64, "seg_ptr")
    if seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
        raise ValueError("seg_ptr: expected [n_seg + 1] offsets")
    n_seg = seg_ptr.numel() - 1
    if ids is not None:
        _chk(ids, I32, "ids")
        if ids.dim() != 1 or ids.numel() != scores.numel():
            raise ValueError(f"ids: {ids.numel()} ids for {scores.numel()} scores")
    eptr = eids_p = None
    if excl is not None:
        if ids is None:
            raise ValueError(f"{name}: excl names item ids, so it needs ids")
        eptr, eids = _rank_csr(excl, n_seg, "excl")
        eids_p = _p(eids) if eids.numel() else _p(eptr)       # every row empty: any valid pointer, nothing is read through it
    if form not in (None, "auto", "wave", "block", 0, 1, 2):
        raise ValueError(f"form={form!r}: expected None / 'auto', 'wave' or 'block'")
    form = {None: 0, "auto": 0, "wave": 1, "block": 2}.get(form, form)
    if max_len is None:
        max_len = int(torch.diff(seg_ptr).max()) if n_seg else 0          # the one synchronisation
    return scores, seg_ptr, n_seg, ids, eptr, eids_p, int(max_len), int(form)


def topk_segments(scores, seg_ptr, k, ids=None, excl=None, max_len=None, form=None, out=None):
    """mvin_topk_segments: the ``k`` best eligible entries of every segment ``scores[seg_ptr[s]:seg_ptr[s+1]]`` of a flat f32
    buffer -- per-user candidate lists of their own lengths -- best first, in topk_rows' order (higher score first, -0.0 equals
    +0.0, NaN below -inf, equal scores by position).  ``seg_ptr`` int64 [n_seg+1]; ``ids`` int32 [T]: every entry's item id, a
    negative id marks padding; ``excl``: a ``(ptr int64 [n_seg+1], ids int32)`` CSR of item ids excluded per segment, each row
    ascending (needs ``ids``).  ``max_len``: an upper bound on the segment lengths; None reads it from ``seg_ptr``, which is ONE
    synchronisation -- with ``max_len`` passed the call only enqueues.  ``form``: None / "auto", "wave" (a segment in the
    registers of a lane group; ``max_len`` <= segments_wave_cap()) or "block" (a workgroup per segment); the numbers do not
    depend on it.  Returns ``(pos int32 [n_seg, k], vals f32 [n_seg, k], ids int32 [n_seg, k] or None, status int64 [2])``
    (``out``: the same four to write into; status is accumulated): positions inside the segment, the input bits of the scores
    and the ids; a segment with fewer than k eligible entries ends in position -1, id -1, value -inf.  A segment longer than
    ``max_len`` is all padding and is counted in status[0] (its k slots in status[1])."""
    lib = _lib.load()
    scores, seg_ptr, n_seg, ids, eptr, eids_p, max_len, form = _segments_common(scores, seg_ptr, ids, excl, max_len, form,
                                                                                 "topk_segments")
    k = int(k)
    if not topk_rows_supported(k):
        raise ValueError(f"k={k}: mvin_topk_segments takes 1 <= k <= 1024")
    dev = scores.device
    if out is None:
        out = (torch.empty((n_seg, k), dtype=I32, device=dev), torch.empty((n_seg, k), dtype=F32, device=dev),
               None if ids is None else torch.empty((n_seg, k), dtype=I32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
    pos, vals, oid, status = out
    _chk(pos, I32, "out pos")
    _chk(vals, F32, "out vals")
    _chk(oid, I32, "out ids")
    _chk(status, torch.int64, "out status")
    if tuple(pos.shape) != (n_seg, k) or tuple(vals.shape) != (n_seg, k) or (oid is not None and tuple(oid.shape) != (n_seg, k)) \
            or (ids is not None and oid is None) or status.numel() != 2:
        raise ValueError(f"out: expected pos / vals / ids [{n_seg}, {k}] (ids with ``ids``) and status [2]")
    T = scores.numel()
    anyp = _p(seg_ptr)                          # an empty array: any valid pointer, nothing is read or written through it
    ids_p = None if ids is None else (_p(ids) if T else anyp)
    _lib.check(lib.mvin_topk_segments(_p(scores) if T else None, T, _p(seg_ptr), n_seg, ids_p, _p(eptr), eids_p, k, max_len, form,
                                      _p(pos) if n_seg else anyp, _p(vals) if n_seg else anyp,
                                      None if ids is None else (_p(oid) if n_seg else anyp), _p(status), _stream()),
               "mvin_topk_segments")
    return pos, vals, oid, status


def rank_segments(scores, seg_ptr, queries, ids=None, excl=None, max_len=None, form=None, out=None):
    """mvin_rank_segments: where named entries of every segment land in the segment's ranking, without ranking it.  ``scores``,
    ``seg_ptr``, ``ids``, ``excl``, ``max_len`` and ``form`` are topk_segments' (``max_len=None`` reads the bound from
    ``seg_ptr``: ONE synchronisation; with ``max_len`` passed the call only enqueues).  ``queries``: a ``(q_ptr int64
    [n_seg+1], q_pos int32 [Q])`` CSR of POSITIONS inside their segments, each row ascending and distinct; ``q_ptr`` holds
    offsets into ``q_pos`` AND into the outputs, so slices ``seg_ptr[s0:s1+1]`` / ``q_ptr[s0:s1+1]`` rank segments s0 .. s1 into
    their places of whole-size outputs.  Returns ``(counts int32 [Q, 3], vals f32 [Q], eligible int32 [n_seg], status int64
    [2])`` (``out``: the same four; status is accumulated) with rank_positives' conventions -- (greater, equal_before,
    equal_after) among the segment's eligible entries and the input bits of the score; (-1, -1, -1) and a quiet NaN for a
    position outside its segment or at an ineligible entry -- so rank_metrics_from_counts takes them as they are.  A segment
    longer than ``max_len`` has every query missing and eligible -1, and is counted in status[0] (its queries in status[1])."""
    lib = _lib.load()
    scores, seg_ptr, n_seg, ids, eptr, eids_p, max_len, form = _segments_common(scores, seg_ptr, ids, excl, max_len, form,
                                                                                 "rank_segments")
    if queries is None or len(queries) != 2:
        raise ValueError("queries: expected a (q_ptr, q_pos) pair")
    qptr, qpos = _rank_csr(queries, n_seg, "queries")
    Q = qpos.numel()
    dev = scores.device
    if out is None:
        out = (torch.empty((Q, 3), dtype=I32, device=dev), torch.empty((Q,), dtype=F32, device=dev),
               torch.empty((n_seg,), dtype=I32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
    counts, vals, eligible, status = out
    _chk(counts, I32, "out counts")
    _chk(vals, F32, "out vals")
    _chk(eligible, I32, "out eligible")
    _chk(status, torch.int64, "out status")
    if tuple(counts.shape) != (Q, 3) or tuple(vals.shape) != (Q,) or tuple(eligible.shape) != (n_seg,) or status.numel() != 2:
        raise ValueError(f"out: expected counts [{Q}, 3], vals [{Q}], eligible [{n_seg}] and status [2]")
    T = scores.numel()
    anyp = _p(seg_ptr)                          # an empty array: any valid pointer, nothing is read or written through it
    ids_p = None if ids is None else (_p(ids) if T else anyp)
    _lib.check(lib.mvin_rank_segments(_p(scores) if T else None, T, _p(seg_ptr), n_seg, ids_p, _p(eptr), eids_p,
                                      _p(qptr), _p(qpos) if Q else anyp, Q, max_len, form, _p(counts) if Q else anyp,
                                      _p(vals) if Q else anyp, _p(eligible) if n_seg else anyp, _p(status), _stream()),
               "mvin_rank_segments")
    return counts, vals, eligible, status


def mmr_max_len():
    """mvin_mmr_max_len: the longest segment mmr_segments takes."""
    return int(_lib.load().mvin_mmr_max_len())


def _mmr_table(feat, name):
    """A feature table checked: (n_rows, D, ld) of an f32 [n_rows, D] tensor with dense rows, rows ``ld`` floats apart."""
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2:
        raise ValueError(f"{name}: expected a [n_rows, D] tensor")
    if feat.dtype != F32:
        raise ValueError(f"{name}: expected an f32 table, got {feat.dtype} (a bf16 table is not taken)")
    n_rows, D = feat.shape
    if D < 4 or D > 256 or D % 4:
        raise ValueError(f"{name}: D={D}: expected a multiple of 4 in 4..256")
    if not feat.is_cuda:
        raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    ld = feat.stride(0) if n_rows > 1 else D
    if feat.stride(1) != 1 or ld < D or ld % 4 or feat.data_ptr() % 16:
        raise ValueError(f"{name}: rows must be dense, a multiple of 4 floats apart and 16-byte aligned")
    return n_rows, D, ld


def row_inv_norms(feat, eps=1e-12, out=None):
    """mvin_row_inv_norms: ``1 / max(||feat[r]||, eps)`` per row of an f32 table [n_rows, D] (rows may be strided), f32 [n_rows]:
    the ``row_scale`` that makes mmr_segments' similarity a cosine.  The sum of squares and the root are taken in f64 and
    rounded once.  Enqueues only."""
    lib = _lib.load()
    eps = float(eps)
    if not (0.0 < eps < 3.0e38):
        raise ValueError(f"eps={eps}: expected a finite value > 0")
    n_rows, D, ld = _mmr_table(feat, "feat")
    if out is None:
        out = torch.empty((n_rows,), dtype=F32, device=feat.device)
    _chk(out, F32, "out")
    if tuple(out.shape) != (n_rows,):
        raise ValueError(f"out: expected [{n_rows}]")
    if n_rows:
        _lib.check(lib.mvin_row_inv_norms(_p(feat), n_rows, D, ld, eps, _p(out), _stream()), "mvin_row_inv_norms")
    return out


def mmr_segments(scores, seg_ptr, ids, feat, k, lam, row_scale=None, excl=None, max_len=None, form=None, out=None):
    """mvin_mmr_segments: greedy maximal-marginal-relevance reranking of every segment ``scores[seg_ptr[s]:seg_ptr[s+1]]`` --
    step t takes, among the eligible entries not taken yet, the largest ``lam * score - (1 - lam) * (largest similarity to
    anything already taken)`` (f32; the first step has no penalty; topk_segments' order, equal values to the lower position).
    ``scores``, ``seg_ptr``, ``excl``, ``max_len`` and ``form`` are topk_segments' (``max_len=None`` reads the bound from
    ``seg_ptr``: ONE synchronisation; with ``max_len`` passed the call only enqueues); ``ids`` int32 [T] is required: an entry's
    id is its row in ``feat`` (f32 [n_rows, D], D a multiple of 4 in 4..256), a negative id is padding and an id >= n_rows is
    ineligible too.  Similarity = the dot product of the two rows, times ``row_scale`` (f32 [n_rows]; ``row_inv_norms(feat)``
    makes it a cosine) of both when given.  LIMITS: 0 <= lam <= 1, 1 <= k <= 1024, segments of at most mmr_max_len() entries.
    Returns ``(pos int32, vals f32, ids int32, mmr f32, pen f32, simsum f32, status int64 [2])``, [n_seg, k] each (``out``: the
    same seven to write into; status is accumulated): per slot the pick's position, the input bits of its score, its id, its
    marginal value, its penalty, and the sum of its similarities to the earlier picks.  A segment short of k eligible entries
    ends in position -1, id -1, value -inf and zeros; a segment over ``max_len`` is all padding and counted in status.  With
    lam = 1 the first three are topk_segments' bit for bit."""
    k, lam = int(k), float(lam)
    if not 1 <= k <= 1024:
        raise ValueError(f"k={k}: mvin_mmr_segments takes 1 <= k <= 1024")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam={lam}: expected a value in [0, 1]")
    if ids is None:
        raise ValueError("mmr_segments: ids is required (an entry's id is its row in feat)")
    n_rows, D, ld = _mmr_table(feat, "feat")
    lib = _lib.load()
    scores, seg_ptr, n_seg, ids, eptr, eids_p, max_len, form = _segments_common(scores, seg_ptr, ids, excl, max_len, form,
                                                                                 "mmr_segments")
    if max_len > mmr_max_len():
        raise ValueError(f"max_len={max_len}: mvin_mmr_segments takes segments of at most {mmr_max_len()} entries")
    if row_scale is not None:
        _chk(row_scale, F32, "row_scale")
        if tuple(row_scale.shape) != (n_rows,):
            raise ValueError(f"row_scale: expected [{n_rows}]")
    dev = scores.device
    if out is None:
        out = tuple(torch.empty((n_seg, k), dtype=dt, device=dev) for dt in (I32, F32, I32, F32, F32, F32)) \
            + (torch.zeros(2, dtype=torch.int64, device=dev),)
    if len(out) != 7:
        raise ValueError("out: expected (pos, vals, ids, mmr, pen, simsum, status)")
    for t, dt, name in zip(out, (I32, F32, I32, F32, F32, F32, torch.int64), ("pos", "vals", "ids", "mmr", "pen", "simsum", "status")):
        _chk(t, dt, f"out {name}")
    if any(t is None or tuple(t.shape) != (n_seg, k) for t in out[:3]) or out[6] is None or out[6].numel() != 2 \
            or any(t is not None and tuple(t.shape) != (n_seg, k) for t in out[3:6]):
        raise ValueError(f"out: expected pos / vals / ids [{n_seg}, {k}], mmr / pen / simsum [{n_seg}, {k}] or None, and status [2]")
    T = scores.numel()
    anyp = _p(seg_ptr)                          # an empty array: any valid pointer, nothing is read or written through it
    opt = lambda t: None if t is None else (_p(t) if n_seg else anyp)      # noqa: E731
    _lib.check(lib.mvin_mmr_segments(_p(scores) if T else None, T, _p(seg_ptr), n_seg, _p(ids) if T else anyp, _p(eptr), eids_p,
                                     _p(feat) if n_rows else None, n_rows, D, ld, _p(row_scale) if n_rows else None, lam, k,
                                     max_len, form, opt(out[0]), opt(out[1]), opt(out[2]), opt(out[3]), opt(out[4]), opt(out[5]),
                                     _p(out[6]), _stream()), "mvin_mmr_segments")
    return tuple(out)


def mips_topk_max_k():
    """mvin_mips_topk_max_k: the largest k the fused retrieval kernel takes."""
    return int(_lib.load().mvin_mips_topk_max_k())


def mips_topk_supported(k, D):
    return bool(_lib.load().mvin_mips_topk_supported(int(k), int(D)))


# Below this many queries form=None takes the composed form.  0: the fused form wherever it is supported.  Set by
# scripts/bench_retrieve.py on the MI355X (48 091 rows, D 64, k 200): fused 0.41 ms against composed
# 0.43 ms at 250 queries (level: 4 %, the spreads 1 % wide) and 7.9 ms against 11.3 ms at 23 553 -- the fused form lost at
# neither end, so no range goes to the composed form.  Other D, k and n have not been measured.
MIPS_FUSED_MIN_QUERIES = 0


def _mips_common(q, feat, cand_ids, col_offset, n, q_scale, row_scale, name):
    """The arguments mips_scores and mips_topk share, checked: (nq, n_rows, D, ld, n, col_offset)."""
    n_rows, D, ld = _mmr_table(feat, "feat")
    if not isinstance(q, torch.Tensor) or q.dim() != 2 or q.shape[1] != D:
        raise ValueError(f"q: expected a [nq, {D}] tensor")
    if q.dtype != F32:
        raise TypeError(f"q: expected {F32}, got {q.dtype}")
    _chk(q, F32, "q")
    if q.data_ptr() % 16:
        raise ValueError("q: rows must be 16-byte aligned")
    nq = q.shape[0]
    col_offset = int(col_offset)
    if cand_ids is not None:
        _chk(cand_ids, I32, "cand_ids")
        if cand_ids.dim() != 1 or (n is not None and int(n) != cand_ids.numel()):
            raise ValueError(f"cand_ids: expected a 1-d tensor of n={n} ids" if n is not None else "cand_ids: expected a 1-d tensor")
        n = cand_ids.numel()
    else:
        if col_offset < 0:
            raise ValueError(f"col_offset={col_offset}: expected >= 0")
        n = max(0, n_rows - col_offset) if n is None else int(n)
        if n < 0 or col_offset + n > 0x7FFFFFFF:
            raise ValueError(f"{name}: n={n} col_offset={col_offset}: implicit ids col_offset + j must be int32")
    for t, size, tname in ((q_scale, nq, "q_scale"), (row_scale, n_rows, "row_scale")):
        if t is not None:
            _chk(t, F32, tname)
            if tuple(t.shape) != (size,):
                raise ValueError(f"{tname}: expected [{size}]")
    return nq, n_rows, D, ld, n, col_offset


def mips_scores(q, feat, cand_ids=None, col_offset=0, n=None, q_scale=None, row_scale=None, out=None):
    """mvin_mips_scores: ``out[i, j] = dot(q[i], feat[row_j])`` (f32 on the matrix cores, one fixed order of d), times
    ``q_scale[i]`` and then ``row_scale[row_j]`` when given.  ``q`` f32 [nq, D]; ``feat`` the f32 table of mmr_segments (rows may
    be strided; a bf16 table is refused); column j is table row ``cand_ids[j]`` (int32 [n]) or ``col_offset + j`` (``n`` columns,
    default: to the end of the table).  A column whose row id is negative or outside the table gets a quiet NaN.  ``out``: f32
    [nq, n], rows may be strided.  Enqueues only."""
    lib = _lib.load()
    nq, n_rows, D, ld, n, col_offset = _mips_common(q, feat, cand_ids, col_offset, n, q_scale, row_scale, "mips_scores")
    if out is None:
        out = torch.empty((nq, n), dtype=F32, device=q.device)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != F32:
        raise TypeError(f"out: expected a CUDA/ROCm {F32} tensor")
    if tuple(out.shape) != (nq, n) or (n > 1 and out.stride(1) != 1) or (nq > 1 and out.stride(0) < n):
        raise ValueError(f"out: expected [{nq}, {n}] with dense rows")
    ldo = out.stride(0) if nq > 1 else n
    if nq and n:
        _lib.check(lib.mvin_mips_scores(_p(q), nq, _p(feat) if n_rows else None, n_rows, D, ld, _p(q_scale), _p(row_scale),
                                        _p(cand_ids), col_offset, n, _p(out), ldo, _stream()), "mvin_mips_scores")
    return out


def _mips_composed(q, feat, k, cand_ids, col_offset, n, n_rows, q_scale, row_scale, excl, max_scores, out):
    """mips_topk's composed form: column blocks of mips_scores into a bounded buffer, topk_rows with its carry."""
    nq, dev = q.shape[0], q.device
    sentinel = 0x7FFFFFFF                       # never a table row (n_rows < 2^31): stands for every ineligible column
    if cand_ids is None:
        n = min(n, max(0, n_rows - col_offset))     # the ineligible columns are the tail
    else:
        # an ineligible column holds a NaN in the dense scores, which topk_rows would rank: give those columns one id and
        # put that id at the end of every exclusion row
        tk_ids = torch.where((cand_ids < 0) | (cand_ids >= n_rows), torch.full_like(cand_ids, sentinel), cand_ids)
        ar = torch.arange(nq + 1, dtype=torch.int64, device=dev)
        if excl is None:
            excl = (ar, torch.full((nq,), sentinel, dtype=I32, device=dev))
        else:
            ptr, ids = excl
            E = ids.numel()
            ids2 = torch.full((E + nq,), sentinel, dtype=I32, device=dev)
            if E:
                rows_of = torch.repeat_interleave(ar[:nq], ptr[1:] - ptr[:-1], output_size=E)
                ids2[torch.arange(E, dtype=torch.int64, device=dev) + rows_of] = ids
            excl = (ptr + ar, ids2)
    blk = max(256, (int(max_scores) // max(nq, 1)) // 256 * 256)
    buf = torch.empty((nq, min(blk, max(n, 1))), dtype=F32, device=dev)
    carry = None
    for b in range(0, max(n, 1), blk):
        w = max(0, min(blk, n - b))
        view = buf[:, :w]
        if cand_ids is None:
            mips_scores(q, feat, None, col_offset + b, w, q_scale, row_scale, out=view)
            carry = topk_rows(view, k, None, col_offset + b, excl, carry, out=out if carry is None else carry)
        else:
            mips_scores(q, feat, cand_ids[b:b + w], 0, None, q_scale, row_scale, out=view)
            carry = topk_rows(view, k, tk_ids[b:b + w], 0, excl, carry, out=out if carry is None else carry)
    return carry


def mips_topk(q, feat, k, cand_ids=None, col_offset=0, n=None, q_scale=None, row_scale=None, excl=None, form=None, splits=0,
              max_scores=1 << 26, out=None):
    """mvin_mips_topk: each query's ``k`` best ELIGIBLE columns of mips_scores(q, feat, ...) -- ``(ids int32 [nq, k], vals f32
    [nq, k])``, the table row and the score, higher first, in topk_rows' order (-0.0 equals +0.0, NaN below -inf, equal scores to
    the lower column), a short row padded with id -1, value -inf.  A column is ineligible when its row id is negative, outside
    the table, or in the query's exclusion row (``excl``: topk_rows' CSR).  ``form="fused"`` selects while it multiplies (no
    [nq, n] buffer; k <= mips_topk_max_k(); ``splits`` > 0 forces the number of column ranges, 0 chooses); ``form="composed"``
    runs column blocks of mips_scores into a buffer of at most ``max_scores`` floats and topk_rows with its carry (k <= 1024);
    ``None`` takes the fused form where it is supported.  Both forms return the same bits.  Enqueues only."""
    lib = _lib.load()
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError(f"k={k}: mvin_mips_topk takes 1 <= k <= 1024")
    if form not in (None, "fused", "composed"):
        raise ValueError(f"form={form!r}: expected None, 'fused' or 'composed'")
    splits = int(splits)
    if not 0 <= splits <= 4096:
        raise ValueError(f"splits={splits}: expected 0 (automatic) or 1 .. 4096")
    nq, n_rows, D, ld, n, col_offset = _mips_common(q, feat, cand_ids, col_offset, n, q_scale, row_scale, "mips_topk")
    if excl is not None:
        ptr, ids = excl
        _chk(ptr, torch.int64, "excl ptr")
        _chk(ids, I32, "excl ids")
        if ptr.numel() != nq + 1:
            raise ValueError(f"excl ptr: {ptr.numel()} entries for {nq} rows")
    if form is None:
        form = "fused" if mips_topk_supported(k, D) and nq >= MIPS_FUSED_MIN_QUERIES else "composed"
    if form == "fused" and not mips_topk_supported(k, D):
        raise ValueError(f"k={k}: the fused form takes k <= {mips_topk_max_k()} (form='composed' takes k <= 1024)")
    dev = q.device
    if out is None:
        out = (torch.empty((nq, k), dtype=I32, device=dev), torch.empty((nq, k), dtype=F32, device=dev))
    oid, oval = out
    _chk(oid, I32, "out ids")
    _chk(oval, F32, "out vals")
    if tuple(oid.shape) != (nq, k) or tuple(oval.shape) != (nq, k):
        raise ValueError(f"out: expected [{nq}, {k}]")
    if nq == 0:
        return oid, oval
    if form == "composed":
        return _mips_composed(q, feat, k, cand_ids, col_offset, n, n_rows, q_scale, row_scale, excl, max_scores, (oid, oval))
    nws = lib.mvin_mips_topk_ws_bytes(nq, n, k, splits)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    eptr = eids = None
    if excl is not None:
        eptr, eids = _p(excl[0]), _p(excl[1]) if excl[1].numel() else _p(excl[0])
    _lib.check(lib.mvin_mips_topk(_p(q), nq, _p(feat) if n_rows else None, n_rows, D, ld, _p(q_scale), _p(row_scale), _p(cand_ids),
                                  col_offset, n, eptr, eids, k, splits, _p(ws), _p(oid), _p(oval), _stream()), "mvin_mips_topk")
    return oid, oval


def mean_rows_segments(feat, ptr, ids, out=None, group=0):
    """mvin_mean_rows_segments: ``out[s]`` = the mean of ``feat[ids[e]]`` over the entries of CSR segment ``s`` (``ptr`` int64
    [n_seg + 1], ``ids`` int32) whose id lies inside the table: each component summed in f64 in entry order, divided by the count
    and rounded to f32 once; a segment without such an entry gives a zero row.  No atomics, so the bits are reproducible and
    independent of ``group`` (lanes per segment: 0 automatic, 8 / 16 / 32 / 64).  Returns f32 [n_seg, D].  Enqueues only."""
    lib = _lib.load()
    n_rows, D, ld = _mmr_table(feat, "feat")
    _chk(ptr, torch.int64, "ptr")
    _chk(ids, I32, "ids")
    if ptr.dim() != 1 or ptr.numel() < 1 or ids.dim() != 1:
        raise ValueError("ptr / ids: expected a CSR pair (ptr int64 [n_seg + 1], ids int32 [total])")
    if group not in (0, 8, 16, 32, 64):
        raise ValueError(f"group={group}: expected 0 (automatic), 8, 16, 32 or 64")
    n_seg = ptr.numel() - 1
    if out is None:
        out = torch.empty((n_seg, D), dtype=F32, device=feat.device)
    _chk(out, F32, "out")
    if tuple(out.shape) != (n_seg, D):
        raise ValueError(f"out: expected [{n_seg}, {D}]")
    if n_seg:
        _lib.check(lib.mvin_mean_rows_segments(_p(feat) if n_rows else None, n_rows, D, ld, _p(ptr), n_seg,
                                               _p(ids) if ids.numel() else _p(ptr), ids.numel(), int(group), _p(out), _stream()),
                   "mvin_mean_rows_segments")
    return out


RESAMPLE_MODES = {"bootstrap": 0, "signflip": 1, "observed": 2}


def resample_max_cols():
    """mvin_resample_max_cols: the columns one mvin_resample_sums launch takes (resample_sums splits wider tables)."""
    return int(_lib.load().mvin_resample_max_cols())


def resample_sums(vals, n_rep, seed=1, mode="bootstrap", first=0, max_groups=0, out=None):
    """mvin_resample_sums: resampled column sums of ``vals`` (f64 [n_rows, n_cols] on the device, dense rows that may be strided;
    one row per user, NaN = undefined for that user) for the replicates ``first .. first + n_rep - 1`` of ``seed``.
    ``mode``: "bootstrap" (n_rows rows drawn with replacement), "signflip" (every row kept, its sign flipped with probability
    1/2) or "observed" (the plain column sums, in the replicates' summation order; seed and replicate are ignored).  ONE draw
    serves every column, so the columns of a call are resampled with the same users.  Returns ``(sums f64 [n_rep, n_cols],
    counts int32 [n_rep, n_cols])`` (``out``: the same two to write into): the sum and the number of the non-NaN cells a
    replicate took per column.  The bits follow the rule in include/mvin_hip.h and depend on neither the other columns, nor
    ``first`` / ``n_rep`` splitting, nor ``max_groups`` (0 automatic, else a cap on the workgroups), nor the row stride.  A table
    wider than resample_max_cols() goes through one launch per block of columns (and one strided copy per block into the
    outputs), which changes no bit.  Enqueues only."""
    lib = _lib.load()
    if not isinstance(vals, torch.Tensor) or vals.dim() != 2:
        raise ValueError("vals: expected a [n_rows, n_cols] tensor")
    if vals.dtype != torch.float64:
        raise TypeError(f"vals: expected torch.float64, got {vals.dtype}")
    if not vals.is_cuda:
        raise _lib.MvinHipError("vals: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if mode not in RESAMPLE_MODES:
        raise ValueError(f"mode={mode!r}: expected one of {sorted(RESAMPLE_MODES)}")
    n_rep, first, max_groups, seed = int(n_rep), int(first), int(max_groups), int(seed)
    if n_rep < 0 or first < 0 or max_groups < 0:
        raise ValueError(f"n_rep={n_rep} first={first} max_groups={max_groups}: expected values >= 0")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed}: expected an unsigned 64-bit value")
    n_rows, n_cols = vals.shape
    ld = vals.stride(0) if n_rows > 1 else max(n_cols, 1)
    if n_rows and ((n_cols > 1 and vals.stride(1) != 1) or ld < n_cols):      # (the strides of an empty dimension say nothing)
        raise ValueError("vals: rows must be dense (stride 1 along the columns, rows at least n_cols doubles apart)")
    if n_rows >= 1 << 31:
        raise ValueError(f"n_rows={n_rows}: mvin_resample_sums takes fewer than 2^31 rows")
    dev = vals.device
    if out is None:
        out = (torch.empty((n_rep, n_cols), dtype=torch.float64, device=dev), torch.empty((n_rep, n_cols), dtype=I32, device=dev))
    if len(out) != 2:
        raise ValueError("out: expected (sums, counts)")
    sums, counts = _chk(out[0], torch.float64, "out sums"), _chk(out[1], I32, "out counts")
    if sums is None or counts is None or tuple(sums.shape) != (n_rep, n_cols) or tuple(counts.shape) != (n_rep, n_cols):
        raise ValueError(f"out: expected sums f64 and counts int32 [{n_rep}, {n_cols}]")
    if n_rep == 0 or n_cols == 0:
        return sums, counts
    cap = resample_max_cols()

    def launch(c0, w, s, c):
        _lib.check(lib.mvin_resample_sums(_p(vals, c0) if n_rows else None, n_rows, w, ld, RESAMPLE_MODES[mode], C.c_uint64(seed), first,
                                          n_rep, max_groups, _p(s), _p(c), _stream()), "mvin_resample_sums")

    if n_cols <= cap:
        launch(0, n_cols, sums, counts)
        return sums, counts
    for c0 in range(0, n_cols, cap):
        w = min(cap, n_cols - c0)
        s = torch.empty((n_rep, w), dtype=torch.float64, device=dev)
        c = torch.empty((n_rep, w), dtype=I32, device=dev)
        launch(c0, w, s, c)
        sums[:, c0:c0 + w].copy_(s)
        counts[:, c0:c0 + w].copy_(c)
    return sums, counts


def resample_summary(obs_sums, obs_counts, sums, counts, level=0.95, num=None, den=None):
    """Intervals from resample_sums' outputs, on the host, per column.  ``obs_sums`` / ``obs_counts`` [n_cols] (or [1, n_cols]):
    the "observed" call; ``sums`` / ``counts`` [R, n_cols]: the bootstrap replicates.  The statistic of a column is its mean
    sum / count -- or, with ``num`` and ``den`` (two equally long lists of column numbers), the ratio sum[num] / sum[den] of two
    column sums (a per-interaction average or an impression-weighted mean under resampling of users).  Returns a dict of f64
    arrays, one entry per column (per ratio): ``mean`` the observed statistic; ``se`` the sample standard deviation (ddof 1) of
    the replicate statistics; ``lo`` / ``hi`` numpy.quantile of the finite replicate statistics at (1 - level) / 2 and
    1 - (1 - level) / 2; ``degenerate`` (int64) the replicates left out because their count (their denominator) was zero.
    NaN where nothing is defined (no finite replicate; ``se`` with fewer than two)."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level={level}: expected a value in (0, 1)")
    if (num is None) != (den is None):
        raise ValueError("num and den go together")
    os_ = np.asarray(obs_sums, dtype=np.float64).reshape(-1)
    oc = np.asarray(obs_counts).astype(np.float64).reshape(-1)
    s = np.asarray(sums, dtype=np.float64)
    c = np.asarray(counts).astype(np.float64)
    if s.ndim != 2 or s.shape != c.shape or s.shape[1] != os_.size or oc.size != os_.size:
        raise ValueError(f"expected sums / counts [R, n_cols] and observed [n_cols], got {s.shape}, {c.shape}, {os_.shape}, {oc.shape}")
    if num is not None:
        num, den = [int(i) for i in num], [int(i) for i in den]
        if len(num) != len(den) or any(not 0 <= i < os_.size for i in num + den):
            raise ValueError("num / den: expected two equally long lists of column numbers")
        top_o, bot_o, top, bot = os_[num], os_[den], s[:, num], s[:, den]
    else:
        top_o, bot_o, top, bot = os_, oc, s, c
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(bot_o != 0, top_o / bot_o, np.nan)
        stat = np.where(bot != 0, top / bot, np.nan)
    n_stat = stat.shape[1]
    out = dict(mean=mean, se=np.full(n_stat, np.nan), lo=np.full(n_stat, np.nan), hi=np.full(n_stat, np.nan),
               degenerate=(bot == 0).sum(axis=0).astype(np.int64))
    a = (1.0 - float(level)) / 2.0
    for j in range(n_stat):
        x = stat[:, j]
        x = x[np.isfinite(x)]
        if x.size:
            out["lo"][j], out["hi"][j] = np.quantile(x, a), np.quantile(x, 1.0 - a)
        if x.size > 1:
            out["se"][j] = np.std(x, ddof=1)
    return out


def signflip_pvalue(obs_sum, sums):
    """The two-sided sign-flip permutation p-value per column: ``(1 + #{r: |sums[r]| >= |obs_sum|}) / (R + 1)`` -- never 0.
    ``obs_sum`` [n_cols] from the "observed" call and ``sums`` [R, n_cols] from the "signflip" call of resample_sums share one
    summation order, so the comparison is exact and ties count.  NaN where the observed sum is NaN."""
    o = np.asarray(obs_sum, dtype=np.float64).reshape(-1)
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != o.size:
        raise ValueError(f"expected sums [R, n_cols] and obs_sum [n_cols], got {s.shape} and {o.shape}")
    with np.errstate(invalid="ignore"):
        p = (1.0 + (np.abs(s) >= np.abs(o)[None, :]).sum(axis=0)) / (s.shape[0] + 1.0)
    return np.where(np.isnan(o), np.nan, p)


def holm_adjust(p):
    """Holm's step-down adjustment of the p-values ``p`` (any shape; the same shape comes back): with the m non-NaN values sorted
    ascending, adjusted_(i) = min(1, max_{j <= i} (m - j + 1) p_(j)).  NaNs pass through and are not counted in m."""
    p = np.asarray(p, dtype=np.float64)
    flat = p.reshape(-1)
    out = np.full(flat.shape, np.nan)
    idx = np.flatnonzero(~np.isnan(flat))
    if idx.size:
        order = idx[np.argsort(flat[idx], kind="stable")]
        m = idx.size
        adj = np.maximum.accumulate((m - np.arange(m)) * flat[order])
        out[order] = np.minimum(1.0, adj)
    return out.reshape(p.shape)


def _score_image_host(vals):
    """mvin_score_image.h on the host: uint32 images of f32 scores (-0.0 = +0.0, every NaN = 0, below image(-inf))."""
    import numpy as np
    u = np.ascontiguousarray(vals, dtype=np.float32).view(np.uint32).astype(np.int64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = np.where(u == 0x80000000, 0, u)
    img = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(nan, 0, img).astype(np.int64)


def _dcg_sum(r):
    """dcg of a 0 / 1 relevance vector, with the operations of harness.dcg_at_k (so that sums agree to the last bit)."""
    import numpy as np
    return float(np.sum(r / np.log2(np.arange(2, r.size + 2)))) if r.size else 0.0


def rank_metrics_from_counts(pos_ptr, counts, eligible, k_list, vals=None, ndcg_window=None):
    """Per-row ranking metrics (float64, on the host) from rank_positives's integers.  ``pos_ptr`` [rows+1], ``counts`` [T, 3],
    ``eligible`` [rows], ``vals`` [T] are host arrays.  Per row: P = its entries (found or not), rho = greater + equal_before of a
    found entry (its 0-based place in the ranking), h_k = #{rho < k}.  Returns a dict of [rows, len(k_list)] arrays:
      precision = h_k / k;  recall = h_k / P (NaN for a row without entries);  hit_ratio = 1.0 if h_k > 0 else 0.0;
      mrr = 1 / (1 + min rho) if min rho < k else 0;  map = (1/k) sum_{i=1..k} h_i / i (the reference's ap_at_k, metrics.py:67-80,
      not the textbook average precision);
      ndcg = the reference's (metrics.py:21-31) over the hit list of the first w = ``ndcg_window`` places (default max(k_list)):
      dcg = sum_{rho < min(k, w)} 1 / log2(rho + 2) over the dcg of min(k, h_w) leading hits, 0 where that is 0 -- with
      w = k_list[-1] what harness._rank_metrics computes, to the last bit;
      ndcg_ideal = the same dcg over the dcg of min(k, P) leading hits (not a number of the reference);
    and, when ``vals`` is given, ``auc`` [rows]: the AUC of the row's found entries against its other eligible columns, ties
    counted half -- NaN where a row has no found entry or no other eligible column, with ONE UndefinedMetricWarning per call."""
    import warnings
    import numpy as np
    ptr = np.asarray(pos_ptr, dtype=np.int64).reshape(-1)
    c = np.asarray(counts).astype(np.int64, copy=False)
    rows = ptr.size - 1
    if rows < 0 or c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"pos_ptr [rows+1] and counts [T, 3] expected, got {ptr.shape} and {c.shape}")
    elig = np.asarray(eligible).astype(np.int64, copy=False).reshape(-1)
    if elig.size != rows:
        raise ValueError(f"eligible: {elig.size} entries for {rows} rows")
    ks = [int(k) for k in k_list]
    if not ks or min(ks) < 1:
        raise ValueError(f"k_list={list(k_list)}: expected at least one k >= 1")
    w = max(ks) if ndcg_window is None else int(ndcg_window)
    if w < 1:
        raise ValueError(f"ndcg_window={ndcg_window}")
    P = np.diff(ptr)
    if rows and (P.min() < 0 or ptr[-1] > c.shape[0] or ptr[0] < 0):
        raise ValueError("pos_ptr: not the offsets of counts")
    sel = np.arange(ptr[0], ptr[-1]) if rows else np.zeros(0, np.int64)
    row_of = np.repeat(np.arange(rows), P)
    c = c[sel]
    found = c[:, 0] >= 0
    rho = np.where(found, c[:, 0] + c[:, 1], np.iinfo(np.int64).max)
    kmax = max(max(ks), w)
    hist = np.zeros((rows, kmax), dtype=np.int64)
    top = rho < kmax
    np.add.at(hist, (row_of[top], rho[top]), 1)
    h = np.cumsum(hist, axis=1)                                    # h[:, i-1] = h_i
    first = np.full(rows, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, row_of, rho)
    out = {m: np.zeros((rows, len(ks)), dtype=np.float64) for m in RANK_METRICS}
    ap_terms = h[:, :max(ks)].astype(np.float64) / np.arange(1, max(ks) + 1, dtype=np.float64)
    ap_sum = np.cumsum(ap_terms, axis=1)                           # sequential, like the reference's loop
    disc = 1.0 / np.log2(np.arange(2, kmax + 2))
    ideal = np.concatenate([[0.0], np.cumsum(disc)])
    with np.errstate(divide="ignore", invalid="ignore"):
        for q, k in enumerate(ks):
            hk = h[:, k - 1]
            out["precision"][:, q] = hk / k
            out["recall"][:, q] = hk / P.astype(np.float64)
            out["hit_ratio"][:, q] = (hk > 0).astype(np.float64)
            out["mrr"][:, q] = np.where(first < k, 1.0 / (1.0 + np.where(first < k, first, 0)), 0.0)
            out["map"][:, q] = ap_sum[:, k - 1] / k
    # ndcg row by row through _dcg_sum: the hit list has min(w, eligible) places, as the ranked list it stands for
    hw = h[:, w - 1] if rows else np.zeros(0, np.int64)
    order = np.argsort(row_of[top], kind="stable")
    rr, pp = row_of[top][order], rho[top][order]
    starts = np.searchsorted(rr, np.arange(rows + 1))
    for r in np.flatnonzero(hw > 0):
        L = int(min(w, elig[r]))
        hits = pp[starts[r]:starts[r + 1]]
        rel = np.zeros(L, dtype=np.float64)
        rel[hits[hits < L]] = 1.0
        for q, k in enumerate(ks):
            cut = rel[:k]
            dcg = _dcg_sum(cut)
            best = np.zeros(cut.size, dtype=np.float64)
            best[:min(k, int(hw[r]))] = 1.0
            idcg = _dcg_sum(best)
            out["ndcg"][r, q] = dcg / idcg if idcg else 0.0
            out["ndcg_ideal"][r, q] = dcg / ideal[min(k, int(P[r]), kmax)]
    if vals is not None:
        v = np.asarray(vals, dtype=np.float32).reshape(-1)[sel]
        img = _score_image_host(v)
        f_row, f_img, f_c = row_of[found], img[found], c[found]
        n_found = np.bincount(f_row, minlength=rows).astype(np.int64)
        n_neg = elig - n_found
        # found entries of the same row above / equal to each found entry, from one sort by (row, image)
        key = f_row * (1 << 32) + f_img
        uniq, inv, cnt_u = np.unique(key, return_inverse=True, return_counts=True)
        end_u = np.cumsum(cnt_u)                                  # entries with key <= uniq[i]
        row_end = np.cumsum(n_found)                              # entries of rows <= r
        pos_above = row_end[f_row] - end_u[inv]
        pos_equal = cnt_u[inv] - 1
        neg_above = f_c[:, 0] - pos_above
        neg_equal = f_c[:, 1] + f_c[:, 2] - pos_equal
        u2 = np.zeros(rows, dtype=np.int64)
        np.add.at(u2, f_row, 2 * (n_neg[f_row] - neg_above) - neg_equal)
        undefined = (n_found == 0) | (n_neg <= 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            auc = np.where(undefined, np.nan, u2.astype(np.float64) / (2.0 * n_found.astype(np.float64) * n_neg.astype(np.float64)))
        out["auc"] = auc
        if undefined.any():
            warnings.warn(f"No found positive or no negative in {int(undefined.sum())} of {rows} row(s): the row's AUC is not "
                          "defined there (NaN)", UndefinedMetricWarning, stacklevel=2)
    return out


def gather_attn_l2_prj(ws, enc_entity, enc_relation, parent_ids, t0, t1, q, B, parents_per_pair, K, D, nR, n_entity, encoded=True, order=None):
    """mvin_gather_attn_l2_prj_fwd: gather_attn_l2_enc over the workspace of ``project_tables`` (built with attention =
    (t0 is not None)).  ``encoded=False``: the two adjacency arrays are the plain adjacency (D = 32, K in {8, 16}).
    Returns (nagg0 [P,D], nagg1 [P,D])."""
    lib = _lib.load()
    for t, dt, nm in ((ws, F32, "ws"), (enc_entity, I32, "enc_entity"), (enc_relation, I32, "enc_relation"),
                      (parent_ids, torch.int64 if parent_ids.dtype == torch.int64 else I32, "parent_ids"), (t0, F32, "t0"),
                      (t1, F32, "t1"), (q, F32, "q")):
        _chk(t, dt, nm)
    if ws.numel() != lib.mvin_project_tables_elems(n_entity, D) or q is None or tuple(q.shape) != (B, D):
        raise ValueError("gather_attn_l2_prj: the workspace of project_tables(n_entity, D) and q [B, D] expected")
    P = B * parents_per_pair
    nagg0 = torch.empty((P, D), dtype=F32, device=ws.device)
    nagg1 = torch.empty((P, D), dtype=F32, device=ws.device)
    _chk(order, I32, "order")
    if order is not None and order.numel() != P:
        raise ValueError("gather_attn_l2_prj: order must be a permutation of the launch's parents")
    _lib.check(lib.mvin_gather_attn_l2_prj_ordered_fwd(_p(ws), _p(enc_entity), _p(enc_relation), 1 if encoded else 0, _p(parent_ids),
                                                       int(parent_ids.dtype == torch.int64), _p(order), _p(t0), _p(t1), _p(q), B,
                                                       parents_per_pair, K, D, n_entity, nR, _p(nagg0), _p(nagg1), _stream()),
               "mvin_gather_attn_l2_prj_fwd")
    return nagg0, nagg1


def gather_attn_l2_agg_supported(D, K, n_entity, nR):
    """mvin_gather_attn_l2_agg_supported: does the per-entity aggregates form take these tables?  (D = 64, K in {16, 32, 64}.)"""
    return bool(_lib.load().mvin_gather_attn_l2_agg_supported(D, K, n_entity, nR))


def entity_aggregates(ws, enc_entity, enc_relation, t0, K, D, nR, n_entity, out=None):
    """mvin_entity_aggregates: S0 | G ([2, n_entity, D] fp32) from the workspace of ``project_tables`` (the CURRENT call's), the
    encoded adjacency and the relation logits t0 of aggregator (0,.) (None: plain mean)."""
    lib = _lib.load()
    for t, dt, nm in ((ws, F32, "ws"), (enc_entity, I32, "enc_entity"), (enc_relation, I32, "enc_relation"), (t0, F32, "t0")):
        _chk(t, dt, nm)
    if ws.numel() != lib.mvin_project_tables_elems(n_entity, D):
        raise ValueError("entity_aggregates: the workspace of project_tables(n_entity, D) expected")
    n = lib.mvin_entity_aggregates_elems(n_entity, D)
    if out is None:
        out = torch.empty((n,), dtype=F32, device=ws.device)
    elif out.numel() != n or out.dtype != F32 or not out.is_contiguous():
        raise ValueError("entity_aggregates: workspace of mvin_entity_aggregates_elems floats expected")
    _lib.check(lib.mvin_entity_aggregates(_p(ws), _p(enc_entity), _p(enc_relation), _p(t0), K, D, n_entity, nR, _p(out), _stream()),
               "mvin_entity_aggregates")
    return out


def gather_attn_l2_agg(ws, agg, enc_entity, enc_relation, parent_ids, t0, t1, q, B, parents_per_pair, K, D, nR, n_entity, order=None):
    """mvin_gather_attn_l2_agg_fwd: gather_attn_l2_prj with the per-entity aggregates of ``entity_aggregates`` beside the
    workspace.  Returns (nagg0 [P,D], nagg1 [P,D])."""
    lib = _lib.load()
    for t, dt, nm in ((ws, F32, "ws"), (agg, F32, "agg"), (enc_entity, I32, "enc_entity"), (enc_relation, I32, "enc_relation"),
                      (parent_ids, torch.int64 if parent_ids.dtype == torch.int64 else I32, "parent_ids"), (t0, F32, "t0"),
                      (t1, F32, "t1"), (q, F32, "q"), (order, I32, "order")):
        _chk(t, dt, nm)
    if (ws.numel() != lib.mvin_project_tables_elems(n_entity, D) or agg.numel() != lib.mvin_entity_aggregates_elems(n_entity, D)
            or q is None or tuple(q.shape) != (B, D)):
        raise ValueError("gather_attn_l2_agg: the workspaces of project_tables / entity_aggregates (n_entity, D) and q [B, D] expected")
    P = B * parents_per_pair
    if order is not None and order.numel() != P:
        raise ValueError("gather_attn_l2_agg: order must be a permutation of the launch's parents")
    nagg0 = torch.empty((P, D), dtype=F32, device=ws.device)
    nagg1 = torch.empty((P, D), dtype=F32, device=ws.device)
    _lib.check(lib.mvin_gather_attn_l2_agg_fwd(_p(ws), _p(agg), _p(enc_entity), _p(enc_relation), _p(parent_ids),
                                               int(parent_ids.dtype == torch.int64), _p(order), _p(t0), _p(t1), _p(q), B,
                                               parents_per_pair, K, D, n_entity, nR, _p(nagg0), _p(nagg1), _stream()),
               "mvin_gather_attn_l2_agg_fwd")
    return nagg0, nagg1


def score_l2_folded_supported(D, K, n_entity, nR):
    """mvin_score_l2_folded_supported: does the folded-tail form take these tables?  (D = 64, K in {16, 32, 64}.)"""
    return bool(_lib.load().mvin_score_l2_folded_supported(D, K, n_entity, nR))


def fold_tables(entity_emb, enc_entity, enc_relation, t0, W0, b0, W1, b1, W2, b2, A0, a0, Wmix, bmix, A1, K, nR, out=None, aggregates=True):
    """mvin_fold_tables: the workspace of the folded-tail form -- TA1 | TA2 | T0A | M0, the aggregates H0 | G and the parameter
    block -- from the CURRENT parameters, the encoded adjacency and the relation logits t0 of aggregator (0,.) (None: plain mean)."""
    lib = _lib.load()
    for t, nm in ((entity_emb, "entity_emb"), (t0, "t0"), (W0, "W0"), (b0, "b0"), (W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2"),
                  (A0, "A0"), (a0, "a0"), (Wmix, "Wmix"), (bmix, "bmix"), (A1, "A1")):
        _chk(t, F32, nm)
    _chk(enc_entity, I32, "enc_entity")
    _chk(enc_relation, I32, "enc_relation")
    nE, D = entity_emb.shape
    n = lib.mvin_fold_tables_elems(nE, D)
    if out is None:
        out = torch.empty((n,), dtype=F32, device=entity_emb.device)
    elif out.numel() != n or out.dtype != F32 or not out.is_contiguous():
        raise ValueError("fold_tables: workspace of mvin_fold_tables_elems floats expected")
    # (aggregates=False: the four per-row tables only -- the workspace of score_l2_folded_gather, where every pair gathers its own rows)
    _lib.check(lib.mvin_fold_tables_ex(_p(entity_emb), _p(enc_entity), _p(enc_relation), _p(t0), _p(W0), _p(b0), _p(W1), _p(b1), _p(W2), _p(b2),
                                       _p(A0), _p(a0), _p(Wmix), _p(bmix), _p(A1), 1 if aggregates else 0, K, D, nE, nR, _p(out), _stream()),
               "mvin_fold_tables")
    return out


def score_l2_folded_gather_supported(D, K, n_entity, nR):
    """mvin_score_l2_folded_gather_supported: the folded tail with every pair gathering its own rows (D = 64, K in {16, 32})."""
    return bool(_lib.load().mvin_score_l2_folded_gather_supported(D, K, n_entity, nR))


def score_l2_folded_gather(ws, enc_entity, enc_relation, items, t0, t1, q, user_o, A1, a1, Wmix, K, D, nR, n_entity, order=None,
                           want_item_emb=True):
    """mvin_score_l2_folded_gather_fwd over the workspace of ``fold_tables(..., aggregates=False)``: (item_emb [B,D] or None, scores [B],
    sigmoid(scores) [B]).  ``order``: a permutation of the pairs (order_by_key over the items) or None."""
    lib = _lib.load()
    for t, dt, nm in ((ws, F32, "ws"), (enc_entity, I32, "enc_entity"), (enc_relation, I32, "enc_relation"),
                      (items, torch.int64 if items.dtype == torch.int64 else I32, "items"), (t0, F32, "t0"), (t1, F32, "t1"), (q, F32, "q"),
                      (user_o, F32, "user_o"), (A1, F32, "A1"), (a1, F32, "a1"), (Wmix, F32, "Wmix"), (order, I32, "order")):
        _chk(t, dt, nm)
    B = items.shape[0]
    if ws.numel() != lib.mvin_fold_tables_elems(n_entity, D) or tuple(q.shape) != (B, D) or tuple(user_o.shape) != (B, D):
        raise ValueError("score_l2_folded_gather: the workspace of fold_tables(n_entity, D) and q, user_o [B, D] expected")
    if order is not None and order.numel() != B:
        raise ValueError("score_l2_folded_gather: order must be a permutation of the pairs")
    item_emb = torch.empty((B, D), dtype=F32, device=ws.device) if want_item_emb else None
    scores = torch.empty((B,), dtype=F32, device=ws.device)
    sig = torch.empty((B,), dtype=F32, device=ws.device)
    i64 = items.dtype == torch.int64
    _lib.check(lib.mvin_score_l2_folded_gather_fwd(_p(ws), _p(enc_entity), _p(enc_relation), _p(items) if i64 else None,
                                                   None if i64 else _p(items), _p(order), _p(t0), _p(t1), _p(q), _p(user_o), _p(A1), _p(a1),
                                                   _p(Wmix), B, K, D, n_entity, nR, _p(item_emb), _p(scores), _p(sig), _stream()),
               "mvin_score_l2_folded_gather_fwd")
    return item_emb, scores, sig


def score_l2_folded(ws, enc_entity, enc_relation, items, t0, t1, q, user_o, A1, a1, Wmix, K, D, nR, n_entity, want_item_emb=True):
    """mvin_score_l2_folded_fwd over the workspace of ``fold_tables``: (item_emb [B,D] or None, scores [B], sigmoid(scores) [B])."""
    lib = _lib.load()
    for t, dt, nm in ((ws, F32, "ws"), (enc_entity, I32, "enc_entity"), (enc_relation, I32, "enc_relation"),
                      (items, torch.int64 if items.dtype == torch.int64 else I32, "items"), (t0, F32, "t0"), (t1, F32, "t1"), (q, F32, "q"),
                      (user_o, F32, "user_o"), (A1, F32, "A1"), (a1, F32, "a1"), (Wmix, F32, "Wmix")):
        _chk(t, dt, nm)
    B = items.shape[0]
    if ws.numel() != lib.mvin_fold_tables_elems(n_entity, D) or tuple(q.shape) != (B, D) or tuple(user_o.shape) != (B, D):
        raise ValueError("score_l2_folded: the workspace of fold_tables(n_entity, D) and q, user_o [B, D] expected")
    two = os.environ.get("MVIN_L2_FOLD_TWO", "0") not in ("", "0")      # (the two-launch A/B variant needs scratch rows for out0 / Z2)
    out0 = torch.empty((B, D), dtype=F32, device=ws.device) if two else None
    z2 = torch.empty((B, D), dtype=F32, device=ws.device) if two else None
    item_emb = torch.empty((B, D), dtype=F32, device=ws.device) if want_item_emb else None
    scores = torch.empty((B,), dtype=F32, device=ws.device)
    sig = torch.empty((B,), dtype=F32, device=ws.device)
    i64 = items.dtype == torch.int64
    _lib.check(lib.mvin_score_l2_folded_fwd(_p(ws), _p(enc_entity), _p(enc_relation), _p(items) if i64 else None, None if i64 else _p(items),
                                            _p(t0), _p(t1), _p(q), _p(user_o), _p(A1), _p(a1), _p(Wmix), B, K, D, n_entity, nR, _p(out0),
                                            _p(z2), _p(item_emb), _p(scores), _p(sig), _stream()), "mvin_score_l2_folded_fwd")
    return item_emb, scores, sig


def gather_mix(table, adj_entity, adj_relation, node_ids, rel_score_t, rowbias, nodes, nodes_per_group, K, nR,
               relu=False):
    """mvin_gather_mix_fwd: out[i] = (1/K) sum_k w_k f(table[adj_entity[x_i,k]] + rowbias[i // npg]) ->
    [nodes, D] fp32 (x_i = node_ids[i], or i when node_ids is None)."""
    lib = _lib.load()
    bf = _chk_table(table, "table")
    for t, dt, nm in ((adj_entity, I32, "adj_entity"), (adj_relation, I32, "adj_relation"),
                      (node_ids, I32, "node_ids"), (rel_score_t, F32, "rel_score"), (rowbias, F32, "rowbias")):
        _chk(t, dt, nm)
    D = table.shape[1]
    out = torch.empty((nodes, D), dtype=F32, device=table.device)
    _lib.check(lib.mvin_gather_mix_fwd(_p(table), _p(adj_entity), _p(adj_relation), _p(node_ids), _p(rel_score_t),
                                       _p(rowbias), nodes, nodes_per_group, K, D, table.shape[0], nR,
                                       1 if relu else 0, _p(out), bf, _stream()), "mvin_gather_mix_fwd")
    return out


def row_softmax(x):
    """mvin_row_softmax_fwd: softmax over the last axis of a [rows, n] fp32 tensor."""
    lib = _lib.load()
    _chk(x, F32, "x")
    out = torch.empty_like(x)
    _lib.check(lib.mvin_row_softmax_fwd(_p(x), x.shape[0], x.shape[1], _p(out), _stream()), "mvin_row_softmax_fwd")
    return out


def mix_neighbor_vectors(neighbor_vectors, neighbor_relations=None, user_embeddings=None, want_probs=False, logits=None):
    """mvin_mix_neighbor_vectors_fwd (aggregators.py:37-77 / :118-152): neighbor_vectors [B,N,K,D] -> mean_k(p * neighbor) [B,N,D]
    (and p [B,N,K]); p = softmax_k(mean_d(user * relation)), or softmax_k(logits [B,N,K]), or 1 when neither is given."""
    lib = _lib.load()
    _chk(neighbor_vectors, F32, "neighbor_vectors")
    B, N, K, D = neighbor_vectors.shape
    if logits is not None:
        _chk(logits, F32, "logits")
        if logits.numel() != B * N * K:
            raise ValueError("logits must be [B,N,K]")
    elif neighbor_relations is not None:
        _chk(neighbor_relations, F32, "neighbor_relations")
        _chk(user_embeddings, F32, "user_embeddings")
        if tuple(neighbor_relations.shape) != (B, N, K, D) or tuple(user_embeddings.shape) != (B, D):
            raise ValueError("neighbor_relations must be [B,N,K,D] and user_embeddings [B,D]")
    out = torch.empty((B, N, D), dtype=F32, device=neighbor_vectors.device)
    probs = torch.empty((B, N, K), dtype=F32, device=neighbor_vectors.device) if want_probs else None
    use_rel = logits is None and neighbor_relations is not None
    _lib.check(lib.mvin_mix_neighbor_vectors_fwd(_p(neighbor_vectors), _p(neighbor_relations) if use_rel else None,
                                                 _p(user_embeddings) if use_rel else None, _p(logits), B, N, K, D,
                                                 _p(out), _p(probs), _stream()), "mvin_mix_neighbor_vectors_fwd")
    return (out, probs) if want_probs else out


def key_addressing_supported(Nm, D):
    return bool(_lib.load().mvin_key_addressing_supported(Nm, D))


def key_addressing(entity_emb, V, w, mem_h, mem_r, mem_t, P, out, ldo, nR):
    """mvin_key_addressing_fwd: every preference-hop attention read of a batch in one launch;
    fills ``out`` [B, ldo] with [o_hset | o_hop0 | ...]."""
    lib = _lib.load()
    bf = _chk_table(entity_emb, "entity_emb")
    _chk(V, F32, "V"), _chk(w, F32, "w"), _chk(out, F32, "out")
    nh = max(1, P)
    arr_t = C.c_void_p * nh
    for lst, nm in ((mem_h[:nh], "mem_h"), (mem_r[:P], "mem_r"), (mem_t[:P], "mem_t")):
        for t in lst:
            _chk(t, I32, nm)
    ph = arr_t(*[t.data_ptr() for t in mem_h[:nh]])
    pr = arr_t(*([t.data_ptr() for t in mem_r[:P]] + [None] * (nh - P)))
    pt = arr_t(*([t.data_ptr() for t in mem_t[:P]] + [None] * (nh - P)))
    B, Nm = mem_h[0].shape
    D = entity_emb.shape[1]
    _lib.check(lib.mvin_key_addressing_fwd(_p(entity_emb), _p(V), _p(w), ph, pr, pt, P, B, Nm, D, nR,
                                           entity_emb.shape[0], _p(out), ldo, bf, _stream()),
               "mvin_key_addressing_fwd")
    return out


def key_addressing_users(entity_emb, V, w, uts, users, P, out, ldo, nR):
    """mvin_key_addressing_users_fwd: key_addressing() with pair b reading the ripple sets of users[b] out of the
    device-resident user_triplet_set ``uts`` [n_user, max(1,P), 3, Nm] int32 (no per-pair [B, Nm] arrays)."""
    lib = _lib.load()
    bf = _chk_table(entity_emb, "entity_emb")
    _chk(V, F32, "V"), _chk(w, F32, "w"), _chk(out, F32, "out"), _chk(uts, I32, "uts")
    if users.dtype not in (torch.int64, I32):
        raise TypeError("users: int64 or int32")
    _chk(users, users.dtype, "users")
    if uts.dim() != 4 or uts.shape[1] != max(1, P) or uts.shape[2] != 3:
        raise ValueError("uts must be [n_user, max(1,P), 3, Nm]")
    B, Nm, D = users.shape[0], uts.shape[3], entity_emb.shape[1]
    u64, u32 = (_p(users), None) if users.dtype == torch.int64 else (None, _p(users))
    _lib.check(lib.mvin_key_addressing_users_fwd(_p(entity_emb), _p(V), _p(w), _p(uts), u64, u32, P, B, Nm, D, nR,
                                                 entity_emb.shape[0], uts.shape[0], _p(out), ldo, bf, _stream()),
               "mvin_key_addressing_users_fwd")
    return out


def l2_tail_supported(D):
    return bool(_lib.load().mvin_l2_tail_supported(D))


def l2_tail(entity_emb, items, q, user_o, nagg0, nagg1, W0, b0, A0, a0, A1, a1, Wmix, bmix):
    """mvin_l2_tail_fwd: projection of level 0, both hop-0 aggregators, the mix-hop combiner and the score in one
    launch (depth-2 trees).  Returns (item_emb [B,D], scores [B], sigmoid [B])."""
    bf = _chk_table(entity_emb, "entity_emb")
    for t, nm in ((q, "q"), (user_o, "user_o"), (nagg0, "nagg0"), (nagg1, "nagg1"), (W0, "W0"), (b0, "b0"), (A0, "A0"),
                  (a0, "a0"), (A1, "A1"), (a1, "a1"), (Wmix, "Wmix"), (bmix, "bmix")):
        _chk(t, F32, nm)
    B, D = user_o.shape
    dev = user_o.device
    i64 = items if items.dtype == torch.int64 else None
    i32 = items if items.dtype == I32 else None
    item_emb = torch.empty((B, D), dtype=F32, device=dev)
    scores = torch.empty((B,), dtype=F32, device=dev)
    sig = torch.empty((B,), dtype=F32, device=dev)
    _lib.check(_lib.load().mvin_l2_tail_fwd(_p(entity_emb), _p(i64), _p(i32), _p(q), _p(user_o), _p(nagg0), _p(nagg1),
                                            _p(W0), _p(b0), _p(A0), _p(a0), _p(A1), _p(a1), _p(Wmix), _p(bmix), B, D,
                                            entity_emb.shape[0], _p(item_emb), _p(scores), _p(sig), bf, _stream()),
               "mvin_l2_tail_fwd")
    return item_emb, scores, sig


def gather_rows(table, ids):
    """mvin_gather_rows: out[i] = table[ids[i]] for rows of any 4-byte-multiple width (fp32 / bf16 entity rows)."""
    _chk(ids, I32, "ids")
    if not table.is_cuda or not table.is_contiguous():
        raise _lib.MvinHipError("table: expected a contiguous CUDA/ROCm tensor")
    out = torch.empty((ids.shape[0], table.shape[1]), dtype=table.dtype, device=table.device)
    _lib.check(_lib.load().mvin_gather_rows(_p(table), _p(ids), ids.shape[0], table.shape[1] * table.element_size(),
                                            _p(out), _stream()), "mvin_gather_rows")
    return out


def scatter_rows(table, ids, rows):
    """mvin_scatter_rows: table[ids[i]] = rows[i] (distinct ids)."""
    _chk(ids, I32, "ids")
    if rows.dtype != table.dtype or not rows.is_contiguous() or not table.is_contiguous():
        raise TypeError("rows/table: same dtype, contiguous")
    _lib.check(_lib.load().mvin_scatter_rows(_p(table), _p(ids), ids.shape[0], table.shape[1] * table.element_size(),
                                             _p(rows), _stream()), "mvin_scatter_rows")
    return table


def shard_space_ids(ids, world, n_local):
    """mvin_shard_space_ids: (ids mod world) * n_local + ids div world, int64 or int32, one launch."""
    if ids.dtype not in (torch.int64, I32) or not ids.is_cuda:
        raise TypeError("ids: int64 or int32 device tensor")
    ids = ids.contiguous()
    out = torch.empty_like(ids)
    _lib.check(_lib.load().mvin_shard_space_ids(_p(ids), int(ids.dtype == torch.int64), ids.numel(), world, n_local,
                                                _p(out), _stream()), "mvin_shard_space_ids")
    return out


def key_addressing_grouped_supported(D, P, Nm, nR):
    return bool(_lib.load().mvin_key_addressing_grouped_supported(D, P, Nm, nR))


def group_sort_ws_elems(n_user, B):
    """int32 words of mvin_group_pairs_by_user's workspace: counters [n_user] | offsets [n_user] | per-pair ranks [B]
    (GroupWs::sort_elems, csrc/mvin_workspaces.h)."""
    return 2 * n_user + B


def score_group_ws_elems(n_user, B):
    """int32 words of mvin_score_l2_args.group_ws, the rule include/mvin_hip.h documents (GroupWs::elems, csrc/mvin_workspaces.h):
    the sort's workspace, then seg_user [B] | seg_ptr [B + 2] | nseg [1] | pair_index [B].  The library exports no function for
    it, so this is the one place on the Python side that states it."""
    return group_sort_ws_elems(n_user, B) + B + (B + 2) + 1 + B


def group_pairs_by_user(users, n_user=None):
    """Segments of a batch in user order, built on the device with static shapes (no host sync, graph-capturable):
    returns (seg_user [B] int32, seg_ptr [B+2] int32, nseg [1] int32, pair_index [B] int32); only the first
    nseg entries of seg_user / nseg+1 of seg_ptr are meaningful.  With ``n_user`` (ids in [0, n_user)):
    mvin_group_pairs_by_user, a counting sort in three small kernels; without: torch.sort + scans."""
    B = users.shape[0]
    if n_user is not None and users.is_cuda and users.dtype in (torch.int64, I32) and users.is_contiguous():
        dev = users.device
        ws = torch.empty(group_sort_ws_elems(n_user, B), dtype=I32, device=dev)
        seg_user = torch.empty(B, dtype=I32, device=dev)
        seg_ptr = torch.empty(B + 2, dtype=I32, device=dev)
        nseg = torch.empty(1, dtype=I32, device=dev)
        pair_index = torch.empty(B, dtype=I32, device=dev)
        u64, u32 = (_p(users), None) if users.dtype == torch.int64 else (None, _p(users))
        _lib.check(_lib.load().mvin_group_pairs_by_user(u64, u32, B, n_user, _p(ws), _p(seg_user), _p(seg_ptr), _p(nseg),
                                                        _p(pair_index), _stream()), "mvin_group_pairs_by_user")
        return seg_user, seg_ptr, nseg, pair_index
    su, perm = torch.sort(users)
    start = torch.ones(B, dtype=torch.bool, device=users.device)
    start[1:] = su[1:] != su[:-1]
    seg_id = torch.cumsum(start, 0) - 1
    nseg = (seg_id[-1:] + 1).to(I32)
    pos = torch.arange(B, dtype=I32, device=users.device)
    seg_ptr = torch.full((B + 2,), B, dtype=I32, device=users.device)
    seg_ptr.scatter_(0, torch.where(start, seg_id, torch.full_like(seg_id, B + 1)), pos)
    seg_user = su[seg_ptr[:B].clamp(max=B - 1).long()].to(I32)
    return seg_user, seg_ptr, nseg, perm.to(I32)


def user_records_len(P, Nm, nR):
    """int32 words of one user's static record (mvin_user_records_len); 0: no record form for this shape."""
    return int(_lib.load().mvin_user_records_len(P, Nm, nR))


def user_records_supported(D, P, Nm, nR, table_bf16=False):
    """True when mvin_key_addressing_grouped_rec_fwd has a kernel over the static records for this shape."""
    return bool(_lib.load().mvin_user_records_supported(D, P, Nm, nR, 1 if table_bf16 else 0))


def build_user_records(uts, P, nR, n_entity):
    """mvin_build_user_records: the static per-user records of ``uts`` [n_user, P, 3, Nm] int32 (relation buckets, tile
    table, clamped head / tail ids) -> [n_user, user_records_len] int32.  Built once per data set, like the adjacency
    encoding: the user's ripple sets are fixed (data_loader_user_set.py), every batch re-reads them."""
    _chk(uts, I32, "uts")
    n_user, Ph, three, Nm = uts.shape
    if Ph != P or three != 3:
        raise ValueError(f"uts shape {tuple(uts.shape)} does not match P={P}")
    n = user_records_len(P, Nm, nR)
    if n == 0:
        raise ValueError(f"no record form for P={P} Nm={Nm} nR={nR}")
    rec = torch.empty((n_user, n), dtype=I32, device=uts.device)
    _lib.check(_lib.load().mvin_build_user_records(_p(uts), n_user, P, Nm, nR, n_entity, _p(rec), _stream()),
               "mvin_build_user_records")
    return rec


def key_addressing_grouped_er_supported(D, P, Nm, nR, n_entity, has_set):
    return bool(_lib.load().mvin_key_addressing_grouped_er_supported(D, P, Nm, nR, n_entity, 1 if has_set else 0))


def project_relations(entity_emb, relation_kge, w=None, out=None):
    """mvin_project_relations: the workspace of the gathered key addressing -- R_KGE[r] . E[e] for every (relation, entity)
    and E[e] . w -- from the CURRENT parameters."""
    lib = _lib.load()
    _chk(entity_emb, F32, "entity_emb"), _chk(relation_kge, F32, "relation_kge"), _chk(w, F32, "w")
    nE, D = entity_emb.shape
    nR = relation_kge.shape[0]
    n = lib.mvin_project_relations_elems(nE, nR, D)
    if out is None:
        out = torch.empty((n,), dtype=F32, device=entity_emb.device)
    elif out.numel() != n or out.dtype != F32 or not out.is_contiguous():
        raise ValueError("project_relations: workspace of mvin_project_relations_elems floats expected")
    _lib.check(lib.mvin_project_relations(_p(entity_emb), _p(relation_kge), _p(w), nE, nR, D, _p(out), _stream()), "mvin_project_relations")
    return out


def key_addressing_grouped(entity_emb, relation_kge, w, uts, groups, items, P, out, ldo, nR, records=None, er=None):
    """mvin_key_addressing_grouped_fwd: the attention reads of a batch whose pairs are grouped by user
    (``groups`` = group_pairs_by_user(users)); fills ``out`` [B, ldo] with [o_hset | o_hop0 | ...].
    ``records`` = build_user_records(uts, ...): the same results from the kernel over static per-user records;
    ``er`` = project_relations(...): that kernel with the users' U rows gathered (mvin_key_addressing_grouped_er_fwd)."""
    lib = _lib.load()
    bf = _chk_table(entity_emb, "entity_emb")
    _chk(relation_kge, F32, "relation_kge"), _chk(w, F32, "w"), _chk(out, F32, "out"), _chk(uts, I32, "uts")
    seg_user, seg_ptr, nseg, perm = groups
    B = items.shape[0]
    n_user, Ph, three, Nm = uts.shape
    D = entity_emb.shape[1]
    i64 = items if items.dtype == torch.int64 else None
    i32 = items if items.dtype == I32 else None
    if i64 is None and i32 is None:
        raise TypeError("items must be int64 or int32")
    if records is not None:
        _chk(records, I32, "records")
        if tuple(records.shape) != (n_user, user_records_len(P, Nm, nR)):
            raise ValueError(f"records shape {tuple(records.shape)} is not that of build_user_records(uts, {P}, {nR}, ...)")
    if er is not None:
        _chk(er, F32, "er")
        if records is None or er.numel() != lib.mvin_project_relations_elems(entity_emb.shape[0], nR, D):
            raise ValueError("key_addressing_grouped: er = project_relations(entity_emb, relation_kge, w) goes with the user records")
        _lib.check(lib.mvin_key_addressing_grouped_er_fwd(_p(entity_emb), _p(relation_kge), _p(w), _p(uts), _p(records), _p(er),
                                                          _p(seg_user), _p(seg_ptr), _p(nseg), _p(perm), _p(i64), _p(i32), B, B, P, Nm, D,
                                                          nR, entity_emb.shape[0], n_user, _p(out), ldo, _stream()),
                   "mvin_key_addressing_grouped_er_fwd")
        return out
    _lib.check(lib.mvin_key_addressing_grouped_rec_fwd(_p(entity_emb), _p(relation_kge), _p(w), _p(uts), _p(records), _p(seg_user),
                                                       _p(seg_ptr), _p(nseg), _p(perm), _p(i64), _p(i32), B, B, P, Nm, D, nR,
                                                       entity_emb.shape[0], n_user, _p(out), ldo, bf, _stream()),
               "mvin_key_addressing_grouped_fwd")
    return out


def key_addressing_flash_supported(D, P, Nm, nR, n_entity):
    return bool(_lib.load().mvin_key_addressing_flash_supported(D, P, Nm, nR, n_entity))


def key_addressing_flash_prepare(entity_emb, relation_kge, w, user_mlp_W, P, out=None):
    """mvin_key_addressing_flash_prepare: the per-call tables of the flash form -- R_KGE[r] . E[e] for every (relation, entity),
    E[e] . w (``w`` None: no h-set read) and E . user_mlp_W[D j : D j + D] per block of o_list -- from the CURRENT parameters."""
    lib = _lib.load()
    for t, nm in ((entity_emb, "entity_emb"), (relation_kge, "relation_kge"), (w, "w"), (user_mlp_W, "user_mlp_W")):
        _chk(t, F32, nm)
    nE, D = entity_emb.shape
    nR = relation_kge.shape[0]
    has_set = w is not None
    if tuple(user_mlp_W.shape) != ((P + (1 if has_set else 0)) * D, D):
        raise ValueError("key_addressing_flash_prepare: user_mlp_W [(P + has_set) D, D] expected")
    n = lib.mvin_key_addressing_flash_tables_elems(nE, nR, D, P, 1 if has_set else 0)
    if out is None:
        out = torch.empty((n,), dtype=F32, device=entity_emb.device)
    elif out.numel() != n or out.dtype != F32 or not out.is_contiguous():
        raise ValueError("key_addressing_flash_prepare: workspace of mvin_key_addressing_flash_tables_elems floats expected")
    _lib.check(lib.mvin_key_addressing_flash_prepare(_p(entity_emb), _p(relation_kge), _p(w), _p(user_mlp_W), nE, nR, D, P, _p(out), _stream()),
               "mvin_key_addressing_flash_prepare")
    return out


def key_addressing_flash(entity_emb, tables, records, groups, items, P, Nm, nR, has_set, user_mlp_b, n_user, sched_ws=None, out=None):
    """mvin_key_addressing_flash_fwd: MVIN._key_addressing + the user MLP for a batch grouped by user (``groups`` =
    group_pairs_by_user(users)) in one barrier-free kernel over the static per-user ``records`` and ``tables`` =
    key_addressing_flash_prepare(entity_emb, relation_kge, w if has_set else None, user_mlp_W, P).  Returns user_o [B, D]."""
    lib = _lib.load()
    for t, dt, nm in ((entity_emb, F32, "entity_emb"), (tables, F32, "tables"), (records, I32, "records"), (user_mlp_b, F32, "user_mlp_b")):
        _chk(t, dt, nm)
    seg_user, seg_ptr, nseg, perm = groups
    B = items.shape[0]
    nE, D = entity_emb.shape
    i64 = items if items.dtype == torch.int64 else None
    i32 = items if items.dtype == I32 else None
    if i64 is None and i32 is None:
        raise TypeError("items must be int64 or int32")
    if tables.numel() != lib.mvin_key_addressing_flash_tables_elems(nE, nR, D, P, 1 if has_set else 0):
        raise ValueError("key_addressing_flash: tables = key_addressing_flash_prepare(entity_emb, relation_kge, w, user_mlp_W, P) expected")
    if tuple(records.shape) != (n_user, user_records_len(P, Nm, nR)):
        raise ValueError(f"records shape {tuple(records.shape)} is not that of build_user_records(uts, {P}, {nR}, ...)")
    n_ws = lib.mvin_key_addressing_flash_ws_elems(B, n_user)
    if sched_ws is None:
        sched_ws = torch.empty((n_ws,), dtype=I32, device=entity_emb.device)
    elif sched_ws.numel() < n_ws or sched_ws.dtype != I32:
        raise ValueError("key_addressing_flash: sched_ws of mvin_key_addressing_flash_ws_elems int32 words expected")
    user_o = out if out is not None else torch.empty((B, D), dtype=F32, device=entity_emb.device)
    _chk(user_o, F32, "out")
    _lib.check(lib.mvin_key_addressing_flash_fwd(_p(entity_emb), _p(tables), _p(records), _p(seg_user), _p(seg_ptr), _p(nseg), _p(perm),
                                                 _p(i64), _p(i32), B, P, Nm, D, nR, nE, n_user, 1 if has_set else 0,
                                                 _p(user_mlp_b), _p(user_o), _p(sched_ws), _stream()),
               "mvin_key_addressing_flash_fwd")
    return user_o


# ------------------------------------------------------------------------------- training ops
def _fill_linear_args(a, srcs, ids, Dout, rows, nz, sum_sources):
    nsrc = len(srcs)
    ids = ids or [None] * nsrc
    ids64 = None
    Dsrc = srcs[0].shape[-1]
    for s in range(nsrc):
        _chk(srcs[s], F32, f"src[{s}]")   # training keeps every table in fp32
        a.src[s] = srcs[s].data_ptr()
        if ids[s] is not None:
            if ids64 is None:
                ids64 = ids[s].dtype == torch.int64
            _chk(ids[s], torch.int64 if ids64 else I32, f"ids[{s}]")
            a.ids[s] = ids[s].data_ptr()
    if rows is None:
        first = next((i for i in ids if i is not None), None)
        rows = first.numel() if first is not None else srcs[0].numel() // Dsrc
    a.nsrc, a.Dsrc, a.Dout, a.rows, a.nz = nsrc, Dsrc, Dout, rows, nz
    a.ids64 = 1 if ids64 else 0
    a.sum_sources = 1 if sum_sources else 0
    return rows


def gather_attn_ex(table, adj_entity, adj_relation, node_ids, rel_score_t, self_vec, Wc, c_child, Wagg, bagg,
                   B, N, K, D):
    """mvin_gather_attn_fwd_ex -> (out, probs | None, s_out, z_out).  ``table``: fp32 or bf16."""
    lib = _lib.load()
    bf = _chk_table(table, "table")
    dev = table.device
    out = torch.empty((B, N, D), dtype=F32, device=dev)
    probs = torch.empty((B, N, K), dtype=F32, device=dev) if rel_score_t is not None else None
    s_out = torch.empty((B * N, D), dtype=F32, device=dev)
    z_out = torch.empty((B * N, D), dtype=F32, device=dev)
    _lib.check(lib.mvin_gather_attn_fwd_ex(_p(table), _p(adj_entity), _p(adj_relation), _p(node_ids), _p(rel_score_t),
                                           _p(self_vec), _p(Wc), _p(c_child), _p(Wagg), _p(bagg), B, N, K, D,
                                           table.shape[0], _p(out), _p(probs), _p(s_out), _p(z_out), bf, _stream()),
               "mvin_gather_attn_fwd_ex")
    return out, probs, s_out, z_out


def agg_ex(self_vec, neigh, rel_ids, rel_score_t, Wagg, bagg, B, N, K, D, want_s=False):
    """mvin_agg_fwd_ex -> (out, probs | None, z_out), or with ``want_s`` (out, probs | None, s_out, z_out)."""
    lib = _lib.load()
    dev = self_vec.device
    out = torch.empty((B, N, D), dtype=F32, device=dev)
    probs = torch.empty((B, N, K), dtype=F32, device=dev) if rel_score_t is not None else None
    s_out = torch.empty((B * N, D), dtype=F32, device=dev) if want_s else None
    z_out = torch.empty((B * N, D), dtype=F32, device=dev)
    _lib.check(lib.mvin_agg_fwd_ex(_p(self_vec), _p(neigh), _p(rel_ids), _p(rel_score_t), _p(Wagg), _p(bagg), B, N, K,
                                   D, _p(out), _p(probs), _p(s_out), _p(z_out), _stream()), "mvin_agg_fwd_ex")
    return (out, probs, s_out, z_out) if want_s else (out, probs, z_out)


def eltwise(mode, n, x, y=None, z=None, w=None, accum=None, alpha=1.0, beta=0.0, beta1=0.0, beta2=0.0, eps=0.0,
            D=1, N=1):
    lib = _lib.load()
    _lib.check(lib.mvin_eltwise(mode, n, _p(x), _p(y), _p(z), _p(w), _p(accum), alpha, beta, beta1, beta2, eps, D, N,
                                _stream()), "mvin_eltwise")


RANK_MODES = {"softmax": 0, "bpr": 1}      # MVIN_RANK_SOFTMAX / MVIN_RANK_BPR


def rank_head(user_o, item_emb, group_size, mode, scale, loss_accum, valid=None, counts=None, out=None, offset=None):
    """mvin_rank_head: the grouped ranking head of the training step in one launch.  ``user_o`` / ``item_emb`` f32 [B, D],
    B = n_groups * ``group_size`` rows group-major (slot 0 of a group the positive, the others negatives of the same user);
    ``valid`` f32 [B] of 0 / 1 (None: every slot counts); ``mode`` "softmax" or "bpr" (include/mvin_hip.h states both).
    Adds ``scale`` * sum of the group losses to ``loss_accum`` (f32 [1]) and, when given, the pairwise-accuracy integers to
    ``counts`` (int64 [2]).  Returns (scores [B], dscore [B], du [B, D], di [B, D]); ``out`` may pass those four buffers in.
    ``offset`` f32 [B] contiguous on the same device (None: no offset, the mvin_rank_head symbol): mvin_rank_head_offset, the
    loss and its gradient are evaluated on score - offset for every valid slot while the scores returned and ``counts`` stay
    on the raw scores (data_prep.rank_offsets builds the logQ correction of a sampled softmax).
    Enqueues only."""
    if mode not in RANK_MODES:
        raise ValueError(f"mode={mode!r}: expected 'softmax' or 'bpr'")
    _chk(user_o, F32, "user_o"), _chk(item_emb, F32, "item_emb"), _chk(loss_accum, F32, "loss_accum")
    _chk(valid, F32, "valid"), _chk(counts, torch.int64, "counts")
    G = int(group_size)
    if user_o.dim() != 2 or tuple(item_emb.shape) != tuple(user_o.shape):
        raise ValueError(f"user_o {tuple(user_o.shape)} and item_emb {tuple(item_emb.shape)}: expected [B, D] both")
    B, D = user_o.shape
    if G < 1 or B % G:
        raise ValueError(f"{B} rows are not whole groups of {G}")
    if valid is not None and valid.numel() != B:
        raise ValueError(f"valid: {valid.numel()} flags for {B} rows")
    if counts is not None and counts.numel() != 2:
        raise ValueError("counts: expected int64 [2]")
    if offset is not None:
        if not torch.is_tensor(offset) or offset.dtype != F32:
            raise ValueError(f"offset: expected a float32 tensor, got {getattr(offset, 'dtype', type(offset))}")
        if offset.numel() != B or offset.device != user_o.device or not offset.is_contiguous():
            raise ValueError(f"offset: expected {B} contiguous values on {user_o.device}, got {tuple(offset.shape)} on "
                             f"{offset.device}")
    if out is None:
        dev = user_o.device
        out = (torch.empty(B, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev),
               torch.empty((B, D), dtype=F32, device=dev), torch.empty((B, D), dtype=F32, device=dev))
    scores, dscore, du, di = out
    for t, nm, n in ((scores, "scores", B), (dscore, "dscore", B), (du, "du", B * D), (di, "di", B * D)):
        _chk(t, F32, nm)
        if t.numel() != n:
            raise ValueError(f"{nm}: {t.numel()} elements, expected {n}")
    if B == 0:                                  # an empty tensor has no address to pass
        return scores, dscore, du, di
    if offset is None:
        _lib.check(_lib.load().mvin_rank_head(_p(user_o), _p(item_emb), _p(valid), B // G, G, D, RANK_MODES[mode], float(scale),
                                              _p(scores), _p(dscore), _p(du), _p(di), _p(loss_accum), _p(counts), _stream()),
                   "mvin_rank_head")
    else:
        _lib.check(_lib.load().mvin_rank_head_offset(_p(user_o), _p(item_emb), _p(valid), _p(offset), B // G, G, D,
                                                     RANK_MODES[mode], float(scale), _p(scores), _p(dscore), _p(du), _p(di),
                                                     _p(loss_accum), _p(counts), _stream()), "mvin_rank_head_offset")
    return scores, dscore, du, di


MF_MODES = {"softmax": 0, "bpr": 1, "bce": 2}   # MVIN_RANK_SOFTMAX / MVIN_RANK_BPR / MVIN_MF_BCE


def _mf_tables(U, V, who):
    for t, nm in ((U, "U"), (V, "V")):
        if not torch.is_tensor(t) or t.dtype != F32 or t.dim() != 2:
            raise ValueError(f"{who}: {nm} must be a float32 [rows, D] tensor, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    D = U.shape[1]
    if V.shape[1] != D or D < 4 or D > 128 or D % 4:
        raise ValueError(f"{who}: U {tuple(U.shape)} and V {tuple(V.shape)}: one D, a multiple of 4 in 4..128")
    if U.shape[0] < 1 or V.shape[0] < 1:
        raise ValueError(f"{who}: empty table (U {tuple(U.shape)}, V {tuple(V.shape)})")
    return D


def _mf_vec(t, name, dtype, n, dev, who):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError(f"{who}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 1 or (n is not None and t.numel() != n) or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{who}: {name}: expected {'' if n is None else n} contiguous values [n] on {dev}, got "
                         f"{tuple(t.shape)} on {t.device}")
    return t


def mf_head(U, V, users, items, mode, scale, reg, loss_accum, group_size=None, valid=None, labels=None, counts=None, out=None,
            grid_cap=0):
    """mvin_mf_head: the head of a matrix-factorisation step in one launch, rows read by id from the tables.  ``U`` f32
    [n_user, D], ``V`` f32 [n_item, D]; ``users`` int64 [n_groups]; ``items`` int64 [B], B = n_groups * ``group_size``
    group-major (slot 0 the positive: the layout of data_prep.rank_groups); ``mode`` "softmax" / "bpr" (group_size 2..64) or "bce"
    (group_size 1, the default there; ``labels`` f32 [B] required, and ``valid`` masks any row).  Adds the loss and the regulariser
    to ``loss_accum`` (f32 [2]) and the pairwise-accuracy integers to ``counts`` (int64 [2], ranking modes).  Returns
    (scores [B], dscore [B], du [B, D], di [B, D]); ``out`` may pass those four in.  include/mvin_hip.h states the rule and the
    bits.  Enqueues only."""
    who = "mf_head"
    if mode not in MF_MODES:
        raise ValueError(f"mode={mode!r}: expected 'softmax', 'bpr' or 'bce'")
    D = _mf_tables(U, V, who)
    dev = U.device
    G = 1 if group_size is None and mode == "bce" else group_size
    if G is None or int(G) != G or not ((G == 1) if mode == "bce" else (2 <= G <= 64)):
        raise ValueError(f"{who}: group_size={group_size!r} (1 for 'bce', 2..64 for the ranking modes)")
    G = int(G)
    users = _mf_vec(users, "users", torch.int64, None, dev, who)
    items = _mf_vec(items, "items", torch.int64, users.numel() * G, dev, who)
    B = items.numel()
    if valid is not None:
        _mf_vec(valid, "valid", F32, B, dev, who)
    if mode == "bce" and labels is None:
        raise ValueError(f"{who}: mode 'bce' needs labels")
    if labels is not None:
        _mf_vec(labels, "labels", F32, B, dev, who)
    _mf_vec(loss_accum, "loss_accum", F32, 2, dev, who)
    if counts is not None:
        _mf_vec(counts, "counts", torch.int64, 2, dev, who)
    _chk(U, F32, "U"), _chk(V, F32, "V")           # the shapes are right: now they must be on the device
    if out is None:
        out = (torch.empty(B, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev),
               torch.empty((B, D), dtype=F32, device=dev), torch.empty((B, D), dtype=F32, device=dev))
    scores, dscore, du, di = out
    for t, nm, n in ((scores, "scores", B), (dscore, "dscore", B), (du, "du", B * D), (di, "di", B * D)):
        _chk(t, F32, nm)
        if t.numel() != n:
            raise ValueError(f"{who}: {nm}: {t.numel()} elements, expected {n}")
    if B == 0:
        return scores, dscore, du, di
    _lib.check(_lib.load().mvin_mf_head(_p(U), U.shape[0], _p(V), V.shape[0], D, _p(users), _p(items), _p(valid), _p(labels),
                                        B // G, G, MF_MODES[mode], float(scale), float(reg), _p(scores), _p(dscore), _p(du), _p(di),
                                        _p(loss_accum), _p(counts), int(grid_cap), _stream()), "mvin_mf_head")
    return scores, dscore, du, di


def mf_scores(U, V, users, items, want_logits=True, want_probs=True):
    """mvin_mf_scores: logits [B] = <U[users], V[items]> with mf_head's bits and probs [B] = their f32 sigmoid, in one launch.
    Returns (logits, probs); one of them is None when not wanted.  Enqueues only."""
    who = "mf_scores"
    D = _mf_tables(U, V, who)
    dev = U.device
    users = _mf_vec(users, "users", torch.int64, None, dev, who)
    items = _mf_vec(items, "items", torch.int64, users.numel(), dev, who)
    if not (want_logits or want_probs):
        raise ValueError(f"{who}: nothing asked for (want_logits and want_probs are both false)")
    _chk(U, F32, "U"), _chk(V, F32, "V")
    B = users.numel()
    logits = torch.empty(B, dtype=F32, device=dev) if want_logits else None
    probs = torch.empty(B, dtype=F32, device=dev) if want_probs else None
    if B:
        _lib.check(_lib.load().mvin_mf_scores(_p(U), U.shape[0], _p(V), V.shape[0], D, _p(users), _p(items), B, _p(logits),
                                              _p(probs), _stream()), "mvin_mf_scores")
    return logits, probs


def sparse_adam_rows(x, m, v, keys, grads, lr_t, beta1, beta2, eps, status, valid=None, order=None, grid_cap=0):
    """mvin_sparse_adam_rows: the lazy Adam over the rows ``keys`` (int64 [n]) name, ``grads`` f32 [n, D] their gradient rows
    (duplicates are summed in ascending index order; include/mvin_hip.h states the rule, exact in numpy float32).  ``x`` / ``m`` /
    ``v`` f32 [n_rows, D] are updated in place; rows no valid key names are not touched.  ``order`` (int32 [n]) defaults to the
    stable ascending sort of ``keys`` (torch.sort: plumbing); ``status`` int64 [2] accumulates (rows updated, entries dropped).
    Enqueues only."""
    who = "sparse_adam_rows"
    for t, nm in ((x, "x"), (m, "m"), (v, "v")):
        if not torch.is_tensor(t) or t.dtype != F32 or t.dim() != 2 or tuple(t.shape) != tuple(x.shape):
            raise ValueError(f"{who}: {nm} must be float32 [n_rows, D] like x, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    n_rows, D = x.shape
    if D < 4 or D > 128 or D % 4:
        raise ValueError(f"{who}: D={D} (a multiple of 4 in 4..128)")
    dev = x.device
    keys = _mf_vec(keys, "keys", torch.int64, None, dev, who)
    n = keys.numel()
    if n >= 1 << 31:
        raise ValueError(f"{who}: {n} keys (order is int32: below 2^31)")
    if not torch.is_tensor(grads) or grads.dtype != F32 or tuple(grads.shape) != (n, D) or grads.device != dev:
        raise ValueError(f"{who}: grads must be float32 [{n}, {D}] on {dev}, got {getattr(grads, 'dtype', type(grads))} "
                         f"{tuple(getattr(grads, 'shape', ()))}")
    if valid is not None:
        _mf_vec(valid, "valid", F32, n, dev, who)
    _mf_vec(status, "status", torch.int64, 2, dev, who)
    _chk(x, F32, "x"), _chk(m, F32, "m"), _chk(v, F32, "v"), _chk(grads, F32, "grads")
    if order is None:
        order = torch.sort(keys, stable=True)[1].to(I32)
    else:
        _mf_vec(order, "order", I32, n, dev, who)
    if n:
        _lib.check(_lib.load().mvin_sparse_adam_rows(_p(x), _p(m), _p(v), n_rows, D, _p(keys), _p(order), _p(grads), _p(valid), n,
                                                     float(lr_t), float(beta1), float(beta2), float(eps), _p(status), int(grid_cap),
                                                     _stream()), "mvin_sparse_adam_rows")
    return order


EXPLAIN_SCALE = float(1 << 40)                 # a mass is floor(w0 * w1 * 2^40); weight = mass / EXPLAIN_SCALE
EXPLAIN_PROFILE_SLOTS = 1 << 22                # B * K * K of one call with rel_mass (mvin_explain_paths' bound)


def explain_paths_max_k():
    """mvin_explain_paths_max_k: the largest fan-out K mvin_explain_paths takes."""
    return int(_lib.load().mvin_explain_paths_max_k())


def explain_paths(imp0, imp1, rels, ents, top, n_relation, rel_mass=None, out=None):
    """mvin_explain_paths: the merged, ranked knowledge-graph attention paths of every pair, in one launch (include/mvin_hip.h
    states the rule).  ``imp0`` f32 [B, 1, K] (or [B, K]) and ``imp1`` f32 [B, K, K] (or [B, K*K]; None = ONE-HOP mode) are the
    attention outputs of the i = 0 pass as ``forward_users(..., want_probs=True).importance_list`` holds them; ``rels`` /
    ``ents`` the int32 id lists of ``MVIN.get_neighbors`` / ``expand_ids`` for the same items: ``rels[0]`` [B, K], ``ents[1]``
    [B, K] and, with ``imp1``, ``rels[1]`` / ``ents[2]`` [B, K*K] (deeper levels are ignored).  Slots that carry the same
    (rel0, ent1, rel1, ent2) are one path: its mass is the int64 sum of floor(w0 * w1 * 2^40) over them, its slot the lowest;
    paths come mass descending, then slot ascending.  ``rel_mass``: int64 [2, n_relation] to ACCUMULATE the per-relation masses
    of both levels into (zero it first; B * K * K <= 2^22 per call).  Returns ``(paths int32 [B, top, 4], mass int64 [B, top],
    slot int32 [B, top], distinct int32 [B], total int64 [B])`` (``out``: the same five to write into); rows past ``distinct``
    hold ids -1, mass 0, slot -1.  Enqueues only."""
    lib = _lib.load()
    for t, name in ((imp0, "imp0"), (imp1, "imp1")):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if imp0 is None:
        raise ValueError("explain_paths: imp0 is required")
    _chk(imp0, F32, "imp0"), _chk(imp1, F32, "imp1"), _chk(rel_mass, torch.int64, "rel_mass")
    two = imp1 is not None
    B, K = imp0.shape[0], imp0.shape[-1]
    N = K * K if two else K
    if imp0.numel() != B * K or (two and (imp1.shape[0] != B or imp1.numel() != B * N)):
        raise ValueError(f"imp0 {tuple(imp0.shape)} / imp1 {None if imp1 is None else tuple(imp1.shape)}: expected [B, 1, K] and [B, K, K]")
    if len(rels) < (2 if two else 1) or len(ents) < (3 if two else 2):
        raise ValueError("rels / ents: expected the lists of get_neighbors (rels[0], ents[1] and, with imp1, rels[1], ents[2])")
    rel0, ent1 = _chk(rels[0], I32, "rels[0]"), _chk(ents[1], I32, "ents[1]")
    rel1, ent2 = (_chk(rels[1], I32, "rels[1]"), _chk(ents[2], I32, "ents[2]")) if two else (None, None)
    for t, n, name in ((rel0, K, "rels[0]"), (ent1, K, "ents[1]"), (rel1, N, "rels[1]"), (ent2, N, "ents[2]")):
        if t is not None and (t.shape[0] != B or t.numel() != B * n):
            raise ValueError(f"{name}: {tuple(t.shape)}, expected [{B}, {n}]")
    top, n_relation = int(top), int(n_relation)
    if not 1 <= K <= explain_paths_max_k() or not 1 <= top <= N:
        raise ValueError(f"K={K} top={top}: mvin_explain_paths takes 1 <= K <= {explain_paths_max_k()} and 1 <= top <= {N}")
    if rel_mass is not None and tuple(rel_mass.shape) != (2, n_relation):
        raise ValueError(f"rel_mass: {tuple(rel_mass.shape)}, expected (2, {n_relation})")
    dev = imp0.device
    if out is None:
        out = (torch.empty((B, top, 4), dtype=I32, device=dev), torch.empty((B, top), dtype=torch.int64, device=dev),
               torch.empty((B, top), dtype=I32, device=dev), torch.empty((B,), dtype=I32, device=dev),
               torch.empty((B,), dtype=torch.int64, device=dev))
    paths, mass, slot, distinct, total = out
    _chk(paths, I32, "out paths"), _chk(mass, torch.int64, "out mass"), _chk(slot, I32, "out slot")
    _chk(distinct, I32, "out distinct"), _chk(total, torch.int64, "out total")
    if tuple(paths.shape) != (B, top, 4) or tuple(mass.shape) != (B, top) or tuple(slot.shape) != (B, top) \
            or tuple(distinct.shape) != (B,) or tuple(total.shape) != (B,):
        raise ValueError(f"out: expected paths [{B}, {top}, 4], mass / slot [{B}, {top}], distinct / total [{B}]")
    if B > 0:                                   # an empty tensor has no address to pass
        _lib.check(lib.mvin_explain_paths(_p(imp0), _p(imp1), _p(rel0), _p(ent1), _p(rel1), _p(ent2), B, K, top, n_relation,
                                          _p(paths), _p(mass), _p(slot), _p(distinct), _p(total), _p(rel_mass), _stream()),
                   "mvin_explain_paths")
    return paths, mass, slot, distinct, total


EXPLAIN_MEM_PROFILE_SLOTS = 1 << 22            # B * Nm of one call with rel_mass (mvin_explain_memories' bound)
EXPLAIN_MEM_OUT = ("mem", "mass", "contrib", "slot", "distinct", "total", "block", "bias")


def explain_memories_max_nm():
    """mvin_explain_memories_max_nm: the largest ripple-set size Nm mvin_explain_memories takes."""
    return int(_lib.load().mvin_explain_memories_max_nm())


def explain_memories(entity_emb, V, w_h, uts, users, G, mlp_bias, item_final, P, top, rel_mass=None, want_slots=False, out=None):
    """mvin_explain_memories: the merged, ranked ripple-set memories behind every pair's user vector, with their signed
    contributions to the logit, in one launch (include/mvin_hip.h states the rule).  ``entity_emb`` f32 [n_entity, D]; ``V`` f32
    [B, nR, D] as MVIN._key_addressing builds it (None when ``P`` == 0); ``w_h`` f32 with at least D entries (None: no h-set
    block); ``uts`` int32 [n_user, max(1, P), 3, Nm]; ``users`` int64 [B]; ``G`` f32 [B, n_o * D] = user_mlp_matrix . v' per
    pair; ``mlp_bias`` f32 [D]; ``item_final`` f32 [B, D].  n_o = P + (w_h is not None).  ``rel_mass``: int64 [P, nR] to
    ACCUMULATE the per-relation masses of the hop blocks into (zero it first; B * Nm <= 2^22 per call).  Returns a dict of
    ``mem`` int32 [B, n_o, top, 3], ``mass`` int64 / ``contrib`` f32 / ``slot`` int32 [B, n_o, top], ``distinct`` int32 /
    ``total`` int64 / ``block`` f32 [B, n_o], ``bias`` f32 [B] and, with ``want_slots``, ``probs`` / ``slot_contrib`` f32
    [B, n_o, Nm] (``out``: such a dict to write into).  Enqueues only."""
    lib = _lib.load()
    for t, name in ((entity_emb, "entity_emb"), (uts, "uts"), (users, "users"), (G, "G"), (mlp_bias, "mlp_bias"),
                    (item_final, "item_final")):
        if not isinstance(t, torch.Tensor):
            raise _lib.MvinHipError(f"{name}: expected a CUDA/ROCm tensor (mvin_amd has no CPU path)")
    if entity_emb.dtype != F32:
        raise ValueError(f"explain_memories: the entity table is {entity_emb.dtype}; mvin_explain_memories takes fp32 tables only")
    P, top = int(P), int(top)
    if entity_emb.dim() != 2 or uts.dim() != 4 or uts.shape[1] != max(1, P) or uts.shape[2] != 3:
        raise ValueError(f"entity_emb {tuple(entity_emb.shape)} / uts {tuple(uts.shape)}: expected [n_entity, D] and "
                         f"[n_user, {max(1, P)}, 3, Nm]")
    (n_entity, D), n_user, Nm, B = entity_emb.shape, uts.shape[0], uts.shape[3], users.numel()
    n_o = P + (1 if w_h is not None else 0)
    if not 0 <= P <= 8 or n_o < 1:
        raise ValueError(f"P={P} with{'' if w_h is not None else 'out'} w_h: mvin_explain_memories takes 0 <= P <= 8 and at least one block")
    if not 1 <= Nm <= explain_memories_max_nm() or not 1 <= top <= Nm or D % 4 or not 4 <= D <= 128:
        raise ValueError(f"Nm={Nm} top={top} D={D}: mvin_explain_memories takes 1 <= Nm <= {explain_memories_max_nm()}, "
                         f"1 <= top <= Nm and D a multiple of 4 in [4, 128]")
    if n_entity < 1 or n_user < 1 or B * n_o * Nm >= 1 << 31:
        raise ValueError(f"n_entity={n_entity} n_user={n_user} B={B}: expected non-empty tables and B * n_o * Nm < 2^31")
    nR = V.shape[1] if V is not None else 0
    if P > 0 and (V is None or V.dim() != 3 or tuple(V.shape) != (B, nR, D) or nR < 1):
        raise ValueError(f"V: {None if V is None else tuple(V.shape)}, expected [{B}, nR, {D}] with P={P}")
    if w_h is not None and w_h.numel() < D:
        raise ValueError(f"w_h: {w_h.numel()} entries, expected at least D={D}")
    if tuple(G.shape) != (B, n_o * D) or tuple(item_final.shape) != (B, D) or mlp_bias.numel() != D:
        raise ValueError(f"G {tuple(G.shape)} / item_final {tuple(item_final.shape)} / mlp_bias {tuple(mlp_bias.shape)}: expected "
                         f"[{B}, {n_o * D}], [{B}, {D}] and [{D}]")
    if rel_mass is not None and (P < 1 or tuple(rel_mass.shape) != (P, nR) or B * Nm > EXPLAIN_MEM_PROFILE_SLOTS):
        raise ValueError(f"rel_mass: {tuple(rel_mass.shape)}, expected ({P}, {nR}) with P >= 1 and B * Nm <= 2^22 per call")
    _chk(entity_emb, F32, "entity_emb"), _chk(V, F32, "V"), _chk(w_h, F32, "w_h"), _chk(uts, I32, "uts")
    _chk(users, torch.int64, "users"), _chk(G, F32, "G"), _chk(mlp_bias, F32, "mlp_bias"), _chk(item_final, F32, "item_final")
    _chk(rel_mass, torch.int64, "rel_mass")         # after the shapes: those are refused the same with and without a GPU
    dev = entity_emb.device
    shapes = dict(mem=((B, n_o, top, 3), I32), mass=((B, n_o, top), torch.int64), contrib=((B, n_o, top), F32),
                  slot=((B, n_o, top), I32), distinct=((B, n_o), I32), total=((B, n_o), torch.int64), block=((B, n_o), F32),
                  bias=((B,), F32))
    if want_slots:
        shapes.update(probs=((B, n_o, Nm), F32), slot_contrib=((B, n_o, Nm), F32))
    if out is None:
        out = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items()}
    for k, (s, d) in shapes.items():
        if k not in out or tuple(out[k].shape) != s:
            raise ValueError(f"out[{k!r}]: expected shape {s}")
        _chk(out[k], d, f"out {k}")
    if B > 0:                                   # an empty tensor has no address to pass
        _lib.check(lib.mvin_explain_memories(_p(entity_emb), _p(V), _p(w_h), _p(uts), _p(users), _p(G), _p(mlp_bias), _p(item_final),
                                             B, P, Nm, D, nR, n_entity, n_user, top, *[_p(out[k]) for k in EXPLAIN_MEM_OUT],
                                             _p(out.get("probs") if want_slots else None),
                                             _p(out.get("slot_contrib") if want_slots else None), _p(rel_mass), _stream()),
                   "mvin_explain_memories")
    return out


def select_negatives(scores, items, valid, n_neg, shortlist, seed, round, group_key=None, counts=None, out_scores=False):
    """mvin_select_negatives: the hard negatives of a ranking objective out of a scored pool, in one launch (include/mvin_hip.h
    states the rule).  ``scores`` f32 / ``items`` int64 / ``valid`` f32 or None, all [n_groups, Gp]: slot 0 of a group is the
    positive, slots 1.. its candidate negatives with the current model's scores.  Of the ``shortlist`` highest-scored valid
    candidates of a group, ``n_neg`` are drawn uniformly as a pure function of (``seed``, ``round``, ``group_key[g]`` -- None:
    g).  Returns (items int64 [n_groups, 1 + n_neg], valid f32 [n_groups, 1 + n_neg]) in the layout of data_prep.rank_groups,
    the chosen hardest first, and with ``out_scores=True`` the chosen slots' score bits as a third tensor (quiet NaN where a
    slot stays unfilled).  ``counts`` (int64 [4]) accumulates the exact integers behind "hard_rate" / "pool_rate".
    Enqueues only."""
    _chk(scores, F32, "scores"), _chk(items, torch.int64, "items"), _chk(valid, F32, "valid")
    _chk(group_key, torch.int64, "group_key"), _chk(counts, torch.int64, "counts")
    if scores is None or items is None:
        raise ValueError("select_negatives: scores and items are required")
    if scores.dim() != 2 or tuple(items.shape) != tuple(scores.shape):
        raise ValueError(f"scores {tuple(scores.shape)} and items {tuple(items.shape)}: expected [n_groups, Gp] both")
    n, Gp = scores.shape
    if valid is not None and tuple(valid.shape) != (n, Gp):
        raise ValueError(f"valid: {tuple(valid.shape)}, expected {(n, Gp)}")
    if group_key is not None and group_key.numel() != n:
        raise ValueError(f"group_key: {group_key.numel()} keys for {n} groups")
    if counts is not None and counts.numel() != 4:
        raise ValueError("counts: expected int64 [4]")
    n_neg, shortlist = int(n_neg), int(shortlist)
    if not 2 <= Gp <= 64 or not 1 <= n_neg <= Gp - 1 or not n_neg <= shortlist <= Gp - 1:
        raise ValueError(f"Gp={Gp} n_neg={n_neg} shortlist={shortlist}: expected 2 <= Gp <= 64, 1 <= n_neg <= shortlist <= Gp - 1")
    dev = scores.device
    out_items = torch.empty((n, 1 + n_neg), dtype=torch.int64, device=dev)
    out_valid = torch.empty((n, 1 + n_neg), dtype=F32, device=dev)
    out_s = torch.empty((n, 1 + n_neg), dtype=F32, device=dev) if out_scores else None
    if n > 0:                                   # an empty tensor has no address to pass
        m64 = (1 << 64) - 1
        _lib.check(_lib.load().mvin_select_negatives(_p(scores), _p(items), _p(valid), _p(group_key), n, Gp, n_neg, shortlist,
                                                     int(seed) & m64, int(round) & m64, _p(out_items), _p(out_valid), _p(out_s),
                                                     _p(counts), _stream()), "mvin_select_negatives")
    return (out_items, out_valid, out_s) if out_scores else (out_items, out_valid)


def count_ids(ids, nbins, out=None):
    """mvin_count_ids: float occurrence counts [nbins] of an int32 id list (no host sync); added to ``out``."""
    _chk(ids, I32, "ids")
    if out is None:
        out = torch.zeros(nbins, dtype=F32, device=ids.device)
    _lib.check(_lib.load().mvin_count_ids(_p(ids), ids.numel(), nbins, _p(out), _stream()), "mvin_count_ids")
    return out


def l2_adam_multi(segs, nseg, total, g, m, v, loss_accum, apply_adam, lr_t, beta1, beta2, eps, lr_dev=None):
    """mvin_l2_adam_multi over the flat gradient / Adam-moment buffers (see include/mvin_hip.h);
    ``lr_dev`` (1-element fp32 device tensor): the step size is read on the device (mvin_l2_adam_multi_dev)."""
    lib = _lib.load()
    for t, nm in ((g, "g"), (m, "m"), (v, "v"), (loss_accum, "loss_accum")):
        _chk(t, F32, nm)
    if lr_dev is not None:
        _chk(lr_dev, F32, "lr_dev")
        _lib.check(lib.mvin_l2_adam_multi_dev(_p(segs), nseg, total, _p(g), _p(m), _p(v), _p(loss_accum),
                                              1 if apply_adam else 0, _p(lr_dev), beta1, beta2, eps, _stream()),
                   "mvin_l2_adam_multi_dev")
        return
    _lib.check(lib.mvin_l2_adam_multi(_p(segs), nseg, total, _p(g), _p(m), _p(v), _p(loss_accum),
                                      1 if apply_adam else 0, lr_t, beta1, beta2, eps, _stream()),
               "mvin_l2_adam_multi")


GUARD_MAX_ITEM = 4096                  # include/mvin_hip.h: MVIN_GUARD_MAX_ITEM
GUARD_MAX_SEG = 256
GUARD_ITEM = np.dtype([("seg", "<i4"), ("len", "<i4"), ("first", "<i8")])                       # mvin_guard_item
GUARD_PARTIAL = np.dtype([("sumsq", "<f8"), ("nonfinite", "<u4"), ("pad", "<u4")])              # mvin_guard_partial
GUARD_STATE = np.dtype([("clip", "<f4"), ("skip", "<i4"), ("ok", "<i4"), ("clipped", "<i4"), ("scale", "<f4"), ("lr_t", "<f4"),
                        ("steps", "<i8"), ("clipped_steps", "<i8"), ("skipped_steps", "<i8"), ("applied", "<i8"),
                        ("last_nonfinite", "<i8"), ("finite_steps", "<i8"), ("norm_sum", "<f8"), ("norm_max", "<f8"), ("last_norm", "<f8"),
                        ("last_sumsq", "<f8"), ("seg_sumsq", "<f8", (GUARD_MAX_SEG,))])         # mvin_guard_state


def guard_work_items(segments):
    """The static work table of mvin_grad_guard for ``segments`` = [(off, n), ...] (flat offset and length, ascending and
    contiguous like mvin_param_seg): items of at most GUARD_MAX_ITEM elements, ascending, none across a segment boundary;
    at most total / GUARD_MAX_ITEM + nseg of them.  A numpy array of GUARD_ITEM."""
    rows = []
    for s, (off, n) in enumerate(segments):
        for first in range(int(off), int(off) + int(n), GUARD_MAX_ITEM):
            rows.append((s, min(GUARD_MAX_ITEM, int(off) + int(n) - first), first))
    return np.array(rows, dtype=GUARD_ITEM)


def grad_guard(segs, nseg, total, g, items, nitems, partials, lr_table, state, grid_cap=0):
    """mvin_grad_guard (see include/mvin_hip.h): ``items`` / ``partials`` / ``state`` are uint8 device tensors holding
    GUARD_ITEM[nitems] / GUARD_PARTIAL[nitems] / one GUARD_STATE, ``lr_table`` the fp32 step sizes of steps 1..T.
    Two launches; enqueues only."""
    _chk(g, F32, "g"), _chk(lr_table, F32, "lr_table")
    for t, nm, need in ((items, "items", nitems * GUARD_ITEM.itemsize), (partials, "partials", nitems * GUARD_PARTIAL.itemsize),
                        (state, "state", GUARD_STATE.itemsize)):
        _chk(t, torch.uint8, nm)
        if t is not None and t.numel() < need:
            raise ValueError(f"grad_guard: {nm} holds {t.numel()} bytes, {need} needed")
    if g is not None and g.numel() < total:
        raise ValueError(f"grad_guard: g holds {g.numel()} floats, total={total}")
    _lib.check(_lib.load().mvin_grad_guard(_p(segs), nseg, total, _p(g), _p(items), nitems, _p(partials), _p(lr_table),
                                           0 if lr_table is None else lr_table.numel(), _p(state), int(grid_cap), _stream()),
               "mvin_grad_guard")


def l2_adam_multi_guarded(segs, nseg, total, g, m, v, loss_accum, apply_adam, state, beta1, beta2, eps):
    """mvin_l2_adam_multi_guarded: ``l2_adam_multi`` with scale, step size and apply / skip read from the GUARD_STATE block
    ``grad_guard`` left (uint8 device tensor)."""
    for t, nm in ((g, "g"), (m, "m"), (v, "v"), (loss_accum, "loss_accum")):
        _chk(t, F32, nm)
    _chk(state, torch.uint8, "state")
    if state is not None and state.numel() < GUARD_STATE.itemsize:
        raise ValueError(f"l2_adam_multi_guarded: state holds {state.numel()} bytes, {GUARD_STATE.itemsize} needed")
    _lib.check(_lib.load().mvin_l2_adam_multi_guarded(_p(segs), nseg, total, _p(g), _p(m), _p(v), _p(loss_accum),
                                                      1 if apply_adam else 0, _p(state), beta1, beta2, eps, _stream()),
               "mvin_l2_adam_multi_guarded")


def axpby(alpha, x, beta, y):
    """y = alpha*x + beta*y (in place on y)."""
    eltwise(0, x.numel(), x, y, alpha=alpha, beta=beta)
    return y


def scatter_add_rows(dtable, ids, x, alpha=1.0):
    lib = _lib.load()
    _chk(dtable, F32, "dtable"), _chk(x, F32, "x")
    D = dtable.shape[-1]
    _lib.check(lib.mvin_scatter_add_rows(_p(dtable), _p(ids), 1 if ids.dtype == torch.int64 else 0, _p(x),
                                         ids.numel(), D, alpha, _stream()), "mvin_scatter_add_rows")


def linear_wgrad(srcs, dY, dW, *, ids=None, db=None, mask=None, sum_sources=False, rows=None, nz=1, ldy=None,
                 dy_zstride=0, ldm=None, mask_zstride=0, dw_zstride=0, db_zstride=0):
    """dW[z] += X^T . dY[z] (X staged like ops.linear), db[z] += column sums."""
    lib = _lib.load()
    a = _lib.LinearArgs()
    Dout = dW.shape[-1]
    _fill_linear_args(a, srcs, ids, Dout, rows, nz, sum_sources)
    ldy = ldy or Dout
    ldm = ldm or Dout
    _lib.check(lib.mvin_linear_wgrad(C.byref(a), _p(dY), ldy, dy_zstride, _p(mask), ldm, mask_zstride, _p(dW),
                                     dw_zstride, _p(db), db_zstride, _stream()), "mvin_linear_wgrad")


def wgrad_problem(srcs, dY, dW, *, ids=None, db=None, mask=None, sum_sources=False, rows=None, nz=1, ldy=None,
                  dy_zstride=0, ldm=None, mask_zstride=0, dw_zstride=0, db_zstride=0):
    """One entry for linear_wgrad_multi (same arguments as linear_wgrad).  Returns (struct, tensors kept alive)."""
    pr = _lib.WgradProblem()
    Dout = dW.shape[-1]
    _fill_linear_args(pr.lin, srcs, ids, Dout, rows, nz, sum_sources)
    pr.dY, pr.ldy, pr.dy_zstride = dY.data_ptr(), ldy or Dout, dy_zstride
    pr.mask, pr.ldm, pr.mask_zstride = (mask.data_ptr() if mask is not None else None), ldm or Dout, mask_zstride
    pr.dW, pr.dw_zstride = dW.data_ptr(), dw_zstride
    pr.db, pr.db_zstride = (db.data_ptr() if db is not None else None), db_zstride
    for t, nm in ((dY, "dY"), (dW, "dW"), (db, "db"), (mask, "mask")):
        _chk(t, F32, nm)
    return pr, (list(srcs), list(ids or ()), dY, dW, db, mask)


def linear_wgrad_multi(problems):
    """mvin_linear_wgrad_multi: the weight gradients of ``problems`` (wgrad_problem entries) in as few launches as
    their shapes allow.  The tensors of every entry must stay alive (and unmodified) until this call."""
    if not problems:
        return
    lib = _lib.load()
    for lo in range(0, len(problems), 64):       # the entry point takes at most 64 problems per call (deep trees queue more)
        chunk = problems[lo:lo + 64]
        arr = (_lib.WgradProblem * len(chunk))(*[p for p, _ in chunk])
        _lib.check(lib.mvin_linear_wgrad_multi(arr, len(chunk), _stream()), "mvin_linear_wgrad_multi")


def agg_bwd(dvec, probs, T, K, D, nR, *, table=None, adj_entity=None, adj_relation=None, node_ids=None, child=None,
            rel_ids=None, dtable=None, dT=None, rel_score=None):
    """mvin_agg_bwd; returns dchild (dense form) or None (gather form: dtable updated in place).
    Gather form with node_ids=None and rel_score given = the by-entity form (dvec is [n_entity, D])."""
    lib = _lib.load()
    dchild = torch.empty((T * K, D), dtype=F32, device=dvec.device) if table is None else None
    _lib.check(lib.mvin_agg_bwd(_p(table), _p(adj_entity), _p(adj_relation), _p(node_ids), _p(child), _p(rel_ids),
                                _p(probs), _p(rel_score), _p(dvec), T, K, D, nR, _p(dtable), _p(dchild), _p(dT),
                                _stream()), "mvin_agg_bwd")
    return dchild


def rel_score_bwd(relation_emb, urh_weights, dT, drel, durh):
    lib = _lib.load()
    nR, D = relation_emb.shape
    _lib.check(lib.mvin_rel_score_bwd(_p(relation_emb), _p(urh_weights), _p(dT), nR, D, _p(drel), _p(durh), _stream()),
               "mvin_rel_score_bwd")


def key_addressing_bwd_adds_item_grad(P, Nm, D, nR):
    return bool(_lib.load().mvin_key_addressing_bwd_adds_item_grad(P, Nm, D, nR))


def key_addressing_bwd(entity_emb, V, w, mem_h, mem_r, mem_t, P, dout, ldo, nR, l2, dE, dV, dw, reg_accum=None,
                       relation_kge=None, items=None):
    """mvin_key_addressing_bwd_reg; ``reg_accum`` (1-element fp32): += l2 * (sum h^2 + sum t^2) of the hop rows;
    ``relation_kge`` + ``items``: the kernel adds dE[item] += sum_r dV[:, r] . R[r]^T itself (see the header)."""
    lib = _lib.load()
    nh = max(1, P)
    arr_t = C.c_void_p * nh
    ph = arr_t(*[t.data_ptr() for t in mem_h[:nh]])
    pr = arr_t(*([t.data_ptr() for t in mem_r[:P]] + [None] * (nh - P)))
    pt = arr_t(*([t.data_ptr() for t in mem_t[:P]] + [None] * (nh - P)))
    B, Nm = mem_h[0].shape
    D = entity_emb.shape[1]
    _lib.check(lib.mvin_key_addressing_bwd_reg(_p(entity_emb), _p(V), _p(w), ph, pr, pt, P, B, Nm, D, nR, _p(dout),
                                               ldo, l2, _p(dE), _p(dV), _p(dw),
                                               1 if dw is None or dw.dim() == 1 else dw.shape[0], _p(reg_accum),
                                               _p(relation_kge), _p(items),
                                               1 if items is not None and items.dtype == torch.int64 else 0, _stream()),
               "mvin_key_addressing_bwd")
