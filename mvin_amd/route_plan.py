"""Which schedule a call takes, how its ripple sets are fed and which key-addressing kernel family runs: decided in ONE place, from
values only (no tensor, no device, no ``ops``), before ``l2_plan`` decides the form of the two deepest levels.

    plan(shape, caps, overrides, thresholds, feed) -> Route(schedule, feed, key_addressing, records, broadcast_user)

schedule: "small" (mvin_score_small_fwd, ONE launch) | "native" (mvin_score_l2_fwd, one call) | "python" (the launches one by one).
feed: "users" (user_triplet_set + user ids, read inside the kernels) | "pairs" (per-pair [B, Nm] lists; also one shared list
replicated because Nm is outside the dense form) | "shared" (one [Nm] list per hop for the whole batch) | "assembled" (per-pair
lists gathered on the device, uts[user]).
key_addressing: "flash" | "gathered_er" | "records" | "grouped" (pairs grouped by user, no static records) | "users_feed" |
"per_pair" | "ripple" (the ops.ripple_attn loop) | "shared" | "none" (the wiring reads no preference set).  For schedule ==
"native" these are ``KeyAddrForm`` of csrc/mvin_score_plan.h in the same order of precedence -- Flash, GatheredER, Records (which
also runs "grouped": the grouped call without a records pointer), UsersFeed, PerPair -- and the library decides again from the
pointers the argument block carries; "small" runs "users_feed" / "per_pair" inside its one launch.
records: the call wants the static per-user records (built once per user_triplet_set tensor, MVIN.user_records).
broadcast_user: a single user id stands for the whole batch.

``MVIN.forward_device`` asks for the route once and dispatches on it; the predicates bench.py and the tests read
(``MVIN._small_ok``, ``_native_l2_ok``, ``_ka_flash_for``, ``_ka_er_for``, ``user_records``) are views of these functions."""
from collections import namedtuple

_THRESHOLDS = dict(
    # up to this many pairs the whole pass is ONE kernel launch (mvin_score_small_fwd: the reference's own batch sizes,
    # 512 / 1024 per sess.run); beyond it the multi-launch schedule is the faster one (measured: 58 vs 60 us at 1 024 pairs,
    # 112 vs 66 us at 2 048: a workgroup walks its pairs' dependent-load chain alone).  The entry point
    # itself takes any batch (tests drive it to 16 384).  0 or MVIN_SMALL=0 turns it off; MVIN_SMALL_MAX overrides
    small_max_batch=1024,
    # that launch addresses the entity table and the adjacency with 32-bit byte offsets
    small_max_table_bytes=(1 << 32) - 4096,
    # above this the pass is kernel-bound: the Python schedule costs nothing
    native_l2_max_batch=65536,
    # grouping pays when users repeat inside the batch (a user's rows are staged once per segment); with
    # about one pair per user the per-pair kernel is the faster one (measured: amazon-shaped, 32 768 pairs
    # of 70 585 users: 15.5 M vs 10.1 M pairs/s).  Static rule, no device sync: pairs per user >= 4.
    group_min_pairs_per_user=4,
    # flash form: its per-call tables cost ~(nR + P + 1) n_entity rows of work whatever the batch (0.15 ms at BASELINE C3, where the
    # kernel then takes 0.52 ms against 0.89 + 0.15 for the kernel over the records + the MLP launch; amazon-book's 39 relations make
    # it a 1.1 GB table): automatic when the users the batch can hold reference at least as many ripple rows as the table has --
    # users x P x Nm >= flash_rows_factor x nR x n_entity
    flash_rows_factor=1,
    # (and never a workspace beyond FLASH_TABLES_MAX_BYTES per stream on its own initiative: nR = 100 relations over 10^6
    #  entities would be a 27 GB table)
    flash_tables_max_bytes=4 << 30,
    # static per-user records: relation buckets, tile table, clamped head / tail ids of every user's ripple sets
    user_records_max_bytes=8 << 30,
    # one shared list per hop: outside the dense form (the [B, Nm] logits go through mvin_linear_fwd) the sets are replicated
    shared_nm_multiple=4, shared_max_nm=256)
THRESHOLDS = namedtuple("Thresholds", list(_THRESHOLDS))(**_THRESHOLDS)

# what the rules read of the model; table_bytes / adj_bytes: the entity table and one adjacency array as stored
RouteShape = namedtuple("RouteShape", "wide_deep PS_only HO_only User_orient_kg_eh PS_O_ft dim K h_hop n_mix_hop p_hop n_memory "
                                      "n_relation n_entity table_f32 table_bytes adj_bytes fused hoist")
# the library's *_supported answers for this shape and table type, gathered once per model; flash_tables_elems: the flash form's
# per-call tables, user_records_words: one user's static record (int32 words)
RouteCaps = namedtuple("RouteCaps", "score_small l2_tail gather_attn_l2 key_addressing key_addressing_grouped user_records "
                                    "key_addressing_flash key_addressing_grouped_er flash_tables_elems user_records_words")
# MVIN.ka_flash (None = automatic) / .ka_er / .static_user_records (False = never) / MVIN_KA_STATIC ("0" = off) /
# .validate_device_ids (ids are checked before the dispatch; the route is the same) / a profile is attached (MVIN._profile) /
# the three batch thresholds as the model holds them (THRESHOLDS has their defaults and measurements)
RouteOverrides = namedtuple("RouteOverrides", "ka_flash ka_er static_user_records ka_static_env validate_device_ids profile "
                                              "small_max_batch native_l2_max_batch group_min_pairs_per_user")
# what the call brought.  kind: "uts" | "pairs" | "shared" | "none"; lists_*: the user_triplet_set, or every per-pair list of the
# first p_hop hops (shape_ok: [n_user, max(1, P), 3, Nm], or [B, Nm] each); n_ids: user ids given; n_user: rows of the
# user_triplet_set; records_ok: the records exist or may be built (the byte cap is met, no graph capture is open)
Feed = namedtuple("Feed", "kind B item_i64 user_i64 user_i32 n_ids lists_i32 lists_contiguous lists_shape_ok n_user distinct_users "
                          "want_probs records_ok")
Route = namedtuple("Route", "schedule feed key_addressing records broadcast_user")

GROUPED_FORMS = ("flash", "gathered_er", "records", "grouped")
RECORD_FORMS = ("flash", "gathered_er", "records")


def need_ps(sh):
    """The wiring reads the preference set (model.py:142-159): key addressing runs at all."""
    return bool(sh.PS_only or not sh.HO_only or sh.User_orient_kg_eh)


def _default_wiring(sh):
    return bool(sh.fused and sh.wide_deep and not sh.PS_only and not sh.HO_only and sh.User_orient_kg_eh and sh.n_mix_hop == 1)


def small_static_ok(sh, caps, th):
    """Everything about ``small_ok`` that does not depend on the call: default wiring, trees of depth 1 or 2, fp32 table below 4 GiB."""
    return bool(_default_wiring(sh) and not sh.hoist and sh.h_hop in (1, 2) and 1 <= sh.p_hop <= 4 and sh.table_f32
                and sh.table_bytes < th.small_max_table_bytes and sh.adj_bytes < th.small_max_table_bytes and caps.score_small)


def small_ok(sh, caps, ov, th, B, item_i64, lists_2d, want_probs):
    """The pass can be ONE kernel launch (mvin_score_small_fwd).  ``lists_2d``: users feed, or per-pair lists."""
    return bool(B <= ov.small_max_batch and not want_probs and not ov.profile and item_i64 and lists_2d and small_static_ok(sh, caps, th))


def native_ok(sh, caps, ov, B, item_i64, lists_2d, want_probs, cap=True):
    """The pass can be enqueued by ONE native call (mvin_score_l2_fwd): default wiring, depth-2 trees."""
    return bool(_default_wiring(sh) and not want_probs and not sh.hoist and not ov.profile and sh.h_hop == 2 and sh.p_hop >= 1
                and item_i64 and lists_2d and caps.l2_tail and caps.gather_attn_l2 and caps.key_addressing
                and (not cap or B <= ov.native_l2_max_batch))


def grouped(sh, caps, ov, lists_ok, B, n_user, distinct_users=None):
    """Pairs grouped by user?  ``lists_ok``: the user_triplet_set is int32 and contiguous."""
    return bool(need_ps(sh) and sh.fused and lists_ok and B >= ov.group_min_pairs_per_user * min(n_user, int(distinct_users or n_user))
                and caps.key_addressing_grouped)


def wants_records(sh, caps, ov, lists_ok, records_ok=True):
    """Static per-user records for this user_triplet_set: where the library has a kernel over them (the records kernel, or the flash
    form on an fp32 table)."""
    if ov.static_user_records is False or ov.ka_static_env == "0" or sh.p_hop < 1 or not lists_ok:
        return False
    return bool((caps.user_records or (sh.table_f32 and caps.key_addressing_flash)) and records_ok)


def flash(sh, caps, ov, th, records, B, n_user, distinct_users=None):
    """Flash form of the grouped key addressing + user MLP (mvin_key_addressing_flash_fwd) for a batch of B pairs?
    ``ov.ka_flash`` True / False (MVIN_KA_FLASH=1 / 0) forces it."""
    if not records or ov.ka_flash is False or not sh.table_f32 or sh.p_hop < 1 or not caps.key_addressing_flash:
        return False
    if ov.ka_flash:
        return True
    if caps.flash_tables_elems * 4 > th.flash_tables_max_bytes:
        return False
    users = min(int(B), int(n_user), int(distinct_users or n_user))
    return users * sh.p_hop * sh.n_memory >= th.flash_rows_factor * sh.n_relation * sh.n_entity


def gathered_er(sh, caps, ov, records):
    """Gathered form of the grouped key addressing?  OFF unless asked for (``MVIN.ka_er = True`` / MVIN_KA_ER=1):
    measured at C3 the kernel over the records goes 0.94 -> 0.74 ms, the table R_KGE[r] . E[e] (245 MB, rebuilt per call) costs
    0.11 ms, and with two scoring streams its writes compete with the other stream's kernels -- 2.74 -> 2.67 ms per step on
    one stream, 197.0 -> 197.6 M pairs/s on two."""
    return bool(ov.ka_er and records and sh.table_f32 and sh.p_hop >= 1 and caps.key_addressing_grouped_er)


def shared_dense(sh, th):
    """One shared list per hop takes the dense form (``MVIN._key_addressing_shared``); else it is replicated per pair."""
    return sh.n_memory % th.shared_nm_multiple == 0 and sh.n_memory <= th.shared_max_nm


def grouped_form(sh, caps, ov, th, fd, schedule):
    """(key-addressing form, records wanted) of a grouped call.  The native call hands the records to the library whenever they
    exist; the Python schedule reaches the kernels over them (plain and gathered) through the records kernel's entry point only."""
    rec = wants_records(sh, caps, ov, fd.lists_i32 and fd.lists_contiguous, fd.records_ok)
    if flash(sh, caps, ov, th, rec, fd.B, fd.n_user, fd.distinct_users):
        return "flash", rec
    usable = rec and (schedule == "native" or caps.user_records)
    if gathered_er(sh, caps, ov, usable):
        return "gathered_er", rec
    return ("records" if rec and caps.user_records else "grouped"), rec


def _pairs(sh, caps, ov, th, fd, feed, lists_ok, broadcast):
    """Per-pair lists, given or assembled: the single launch, the native call, else the per-pair kernel / the ripple_attn loop."""
    if lists_ok and small_ok(sh, caps, ov, th, fd.B, fd.item_i64, True, fd.want_probs):
        return Route("small", feed, "per_pair", False, broadcast)
    if lists_ok and native_ok(sh, caps, ov, fd.B, fd.item_i64, True, fd.want_probs):
        return Route("native", feed, "per_pair", False, broadcast)
    return Route("python", feed, _per_pair(sh, caps), False, broadcast)


def _per_pair(sh, caps):
    return "none" if not need_ps(sh) else "per_pair" if sh.fused and caps.key_addressing else "ripple"


def plan(sh, caps, ov, th, fd):
    """The route of one call."""
    ps = need_ps(sh)
    if fd.kind == "shared":
        broadcast = fd.n_ids == 1
        if not shared_dense(sh, th):
            return Route("python", "pairs", _per_pair(sh, caps), False, broadcast)
        return Route("python", "shared", "shared" if ps else "none", False, broadcast)
    if fd.kind != "uts":
        return _pairs(sh, caps, ov, th, fd, "pairs", fd.kind == "pairs" and fd.lists_i32 and fd.lists_contiguous and fd.lists_shape_ok, False)
    broadcast = fd.n_ids == 1 and fd.B > 1
    ids_ok = broadcast or fd.n_ids == fd.B
    lists_ok = fd.lists_i32 and fd.lists_contiguous
    grp = grouped(sh, caps, ov, lists_ok, fd.B, fd.n_user, fd.distinct_users)
    if ps and lists_ok and fd.lists_shape_ok and fd.user_i64 and ids_ok:
        if small_ok(sh, caps, ov, th, fd.B, fd.item_i64, True, fd.want_probs):
            return Route("small", "users", "users_feed", False, broadcast)
        # (grouped: any batch size -- the host issues ONE call per step instead of seven)
        if native_ok(sh, caps, ov, fd.B, fd.item_i64, True, fd.want_probs, cap=not grp):
            form, rec = grouped_form(sh, caps, ov, th, fd, "native") if grp else ("users_feed", False)
            return Route("native", "users", form, rec, broadcast)
    if not ps:
        return Route("python", "users", "none", False, broadcast)
    if grp:
        form, rec = grouped_form(sh, caps, ov, th, fd, "python")
        return Route("python", "users", form, rec, broadcast)
    # the Python schedule of the users feed (batches above native_l2_max_batch, int32 user ids, sharded tables)
    if sh.fused and lists_ok and fd.lists_shape_ok and ids_ok and (fd.user_i64 or fd.user_i32) and caps.key_addressing:
        return Route("python", "users", "users_feed", False, broadcast)
    # any other wiring: the per-pair feeds are assembled on the device (contiguous, of the user_triplet_set's dtype)
    return _pairs(sh, caps, ov, th, fd, "assembled", fd.lists_i32 and fd.lists_shape_ok and ids_ok, broadcast)
