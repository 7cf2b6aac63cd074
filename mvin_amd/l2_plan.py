"""Which kernel form the two deepest tree levels take for a call: decided in ONE place, from values only (no tensor, no device).

    plan(shape, overrides, caps, thresholds, distinct_fraction, B, n_parents, ...) -> L2Plan(adjacency, form, item_order)

adjacency: "plain" | "encoded" (the duplicate-slot encoding); form: "unprojected" | "tables" (mvin_project_tables) | "aggregates"
(+ mvin_entity_aggregates) | "folded" (mvin_fold_tables -> mvin_score_l2_folded_fwd) | "folded_gather" (the folded tail, every pair
gathering its own rows); item_order: the launch's parents go in item order (mvin_order_by_key).  Both schedules of ``MVIN`` ask for
the plan once and branch on it; the predicates bench.py and the tests read (``MVIN._enc_for_l2`` ...) are views of these functions."""
from collections import namedtuple

_THRESHOLDS = dict(
    # a sampled adjacency repeats slots whenever deg < K (data_loader_user_set.py:383-384); the packed-tile fused kernel walks the
    # distinct slots only.  It pays when rows repeat: below this mean fraction of distinct slots per row it is taken ("auto")
    enc_auto_max_distinct_fraction=0.75,
    # below: a few tiles per workgroup, the pipeline's fill / drain dominates (B = 512: 68 vs 58 us)
    enc_auto_min_parents=2048,
    # measured (scripts/ab_enc.sh): the wave-per-parent kernel keeps D = 32, K <= 16 (BASELINE C2: 1.53 vs 1.88 ms) ... unless the call
    # takes the folded tail over per-entity aggregates, which reads the encoding (C2 at bench size): children >= 10 n_entity
    enc_d32_max_k=16, enc_d32_fold_factor=10,
    # item order: batches large enough to hold repeated items (the launch's requests past the L2 halve at BASELINE C3, 7.5 -> 3.6 GB,
    # and those bytes are what bounds the step; mvin_order_by_key costs ~36 us per 524 288 pairs)
    item_order_min_batch=32768,
    # projected tables, automatic: children (parents x K) >= factor x n_entity.  Measured break-even (pairs per step, one GPU) with the
    # aggregates / the folded tail behind the tables: C3 (K = 32) ~32 768 = 10 n_entity / K, C4 (K = 64) ~8 192 = 4.6 n_entity / K;
    # the kernels over the tables themselves: 16
    prj_factor_tables=16, prj_factor_aggregates=10, prj_factor_aggregates_k64=5,
    # offsets: projected tables and the batch's rows below 1 GiB; the encoded kernels address the table with 32-bit offsets (4 GiB),
    # the adjacency and their output rows with signed ones (2 GiB, fused_packed_applies)
    prj_max_bytes=1 << 30, enc_max_table_bytes=1 << 32, enc_max_offset_bytes=1 << 31)
THRESHOLDS = namedtuple("Thresholds", list(_THRESHOLDS))(**_THRESHOLDS)

# model shape: depth = n_mix_hop * h_hop, table_bytes = the entity table as stored
L2Shape = namedtuple("L2Shape", "dim K depth n_entity n_relation table_f32 table_bytes user_orient fused")
# MVIN.prj / .agg / .fold / .item_order (None = automatic); "0" | "1" | else automatic of MVIN.dedup / MVIN_L2_ENC; MVIN_L2_WPP != "0"
L2Overrides = namedtuple("L2Overrides", "prj agg fold enc_mode item_order wpp")
# the library's *_supported answers for these tables: encoding, projected tables over the PLAIN adjacency, aggregates, folded tail, its gather form
L2Caps = namedtuple("L2Caps", "enc prj_plain agg fold fold_gather")
L2Plan = namedtuple("L2Plan", "adjacency form item_order")


def encoded(sh, ov, caps, th, distinct_fraction, n_parents=None, want_probs=False):
    """The encoded adjacency (packed-tile kernel) for a call over ``n_parents`` level-(L-2) nodes?  ``distinct_fraction``: the
    adjacency's mean fraction of distinct slots per row, None = there is no encoding."""
    mode = ov.enc_mode
    if mode == "0" or want_probs or sh.fused is False:
        return False
    if mode != "1":
        if sh.dim == 32 and sh.K <= th.enc_d32_max_k and not (
                n_parents is not None and sh.depth == 2 and sh.user_orient and ov.fold is not False and ov.agg is not False
                and ov.prj is not False and sh.table_f32 and n_parents * sh.K >= th.enc_d32_fold_factor * sh.n_entity and caps.fold):
            return False
        if n_parents is not None and n_parents < th.enc_auto_min_parents:
            return False
    if sh.table_bytes >= th.enc_max_table_bytes or sh.n_entity * sh.K * 4 >= th.enc_max_offset_bytes or (
            n_parents is not None and n_parents * sh.dim * 4 >= th.enc_max_offset_bytes):
        return False
    return distinct_fraction is not None and (mode == "1" or distinct_fraction <= th.enc_auto_max_distinct_fraction)


def projected_plain(sh, caps):
    """Projected tables over the PLAIN adjacency: the wave-per-parent kernel of D = 32, K in {8, 16} (BASELINE C2), where the library
    takes THAT kernel for these tables (the relation logits fit its LDS, adjacency < 2 GiB, MVIN_L2_D32 does not forbid it)."""
    return bool(sh.dim == 32 and sh.K in (8, 16) and sh.fused is not False and sh.table_f32 and caps.prj_plain)


def projected(sh, ov, caps, th, B, n_parents=None):
    """Projected-tables form for a batch of B pairs (``n_parents`` level-(L-2) nodes)?  ``ov.prj``: None = automatic."""
    if not (sh.user_orient and sh.table_f32 and sh.table_bytes < th.prj_max_bytes and B * sh.dim * 4 < th.prj_max_bytes):
        return False
    if ov.prj is not None:
        return bool(ov.prj)
    # D <= 64, K <= 32: the other instances of the kernel are at their register budget already (K = 64: the second self row costs 18
    # spilled registers) and measured no faster (C4); K = 64 takes it where the aggregates exist (the tables are only their input)
    aggs = ov.agg is not False and ((sh.dim == 64 and caps.agg) or (sh.dim == 32 and sh.depth == 2 and ov.fold is not False and caps.fold))
    factor = (th.prj_factor_aggregates_k64 if sh.K == 64 else th.prj_factor_aggregates) if aggs else th.prj_factor_tables
    return bool(sh.dim <= 64 and (sh.K <= 32 or (sh.K == 64 and aggs)) and (n_parents or B) * sh.K >= factor * sh.n_entity)


def aggregates(ov, caps, enc):
    """Per-entity aggregates behind the tables (~17 gathered rows per entity save a parent ~100 of its ~120 at C3): whenever the
    tables themselves pay, on the shapes the kernels take (D = 64, K in {16, 32, 64}, encoded adjacency)."""
    return bool(enc and ov.agg is not False and caps.agg)


def folded(sh, ov, caps, enc):
    """Folded tail (six products per pair instead of eight) wherever the aggregates form is taken on a depth-2 tree, User_orient on."""
    return bool(enc and ov.fold is not False and ov.agg is not False and sh.user_orient and caps.fold)


def item_order(sh, ov, th, B):
    """Parents in item order?  For the wave-per-parent kernel (dim 64, fan-out <= 32, depth-2 trees: the parents are the pairs)."""
    want = B >= th.item_order_min_batch if ov.item_order is None else ov.item_order
    return bool(sh.dim == 64 and sh.K <= 32 and sh.depth == 2 and ov.wpp and want)


def plan(sh, ov, caps, th, distinct_fraction, B, n_parents, want_probs=False, use_tail=True, gather_form=True):
    """The form of the two deepest levels for one call.  Where the two schedules differ on purpose, the caller says so:
    ``n_parents``: the native call passes B (depth-2 trees only), the Python schedule B K^(L-2);
    ``use_tail``: the one-launch tail applies (depth 2, one mix hop; always so for the native call): the folded form IS that tail;
    ``gather_form``: the schedule has the gather form of the folded tail (mvin_score_l2_fwd has it, the Python schedule has not)."""
    enc = encoded(sh, ov, caps, th, distinct_fraction, n_parents, want_probs)
    form = "unprojected"
    # (the projected-tables kernels write no attention outputs: a want_probs pass keeps the form that does)
    if not want_probs and (enc or projected_plain(sh, caps)) and projected(sh, ov, caps, th, B, n_parents):
        if use_tail and folded(sh, ov, caps, enc):
            form = "folded"
        # MVIN.agg = False ("every pair gathers its own rows"): the folded tail still applies, in its gather form
        elif gather_form and enc and ov.agg is False and ov.fold is not False and sh.user_orient and sh.depth == 2 and caps.fold_gather:
            form = "folded_gather"
        else:
            form = "aggregates" if aggregates(ov, caps, enc) else "tables"
    # (the aggregates form gathers ~12 rows of a 27 MB table per pair: item order buys it nothing -- measured 235 vs 252 us at C3)
    order = bool(enc and form in ("tables", "folded_gather") and item_order(sh, ov, th, B))
    return L2Plan("encoded" if enc else "plain", form, order)
