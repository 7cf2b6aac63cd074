"""-m gpu: which schedule a call takes, how its ripple sets are fed and which key-addressing form runs, replayed against a recording.

tests/golden/route_plan_cases.json holds, for a grid in which every routing rule flips once (just below and at its threshold), what a
forward did at the boundary to the library: the ordered ``mvin_amd.ops`` calls of key addressing, which of mvin_score_small_fwd /
mvin_score_l2_fwd was called and which feed / key-addressing pointers its argument block carried, and what every routing view of
``MVIN`` answered.  It was recorded with ``record_model`` below on the commit before the routing moved into
``mvin_amd/route_plan.py`` (the hash is in the file); the replay asserts that nothing moved, and that every case's scores agree
with the fp32 mirror of the reference graph.  Measured on an MI355X: the 13 models' 225 cases replay in 2.9 s together, the slowest
model (h3, the per-level kernels at 2 048 pairs) in 1.1 s, the main model's 89 cases in 0.5 s."""
import json
import os

import numpy as np
import pytest
import torch

from mvin_amd import _lib, ops, synth
from mvin_amd.config import make_args
from mvin_amd.model import MVIN
from mvin_amd.params import init_params

from parity import assert_close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_plan_cases.json")
N_ENTITY, N_RELATION, N_USER, N_COMBOS = 96, 5, 32, 96          # batch row b holds combo b % N_COMBOS, the mirror runs once over them
SHAPE = dict(dim=64, neighbor_sample_size=16, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=16)

TRACED = ("key_addressing", "key_addressing_users", "key_addressing_grouped", "key_addressing_flash_prepare", "key_addressing_flash",
          "project_relations", "ripple_attn", "build_user_records", "group_pairs_by_user", "row_softmax")
NATIVE = ("mvin_score_small_fwd", "mvin_score_l2_fwd")
ARG_POINTERS = ("uts", "mem_h", "user_records", "ka_flash", "ka_er", "group_ws")
BASE = dict(ka_flash=None, ka_er=False, static_user_records=None, fused=True, hoist=False, validate_device_ids=False, _profile=None,
            small_max_batch=1024, native_l2_max_batch=65536, group_min_pairs_per_user=4)
SMALL_OFF, PROFILE = dict(small_max_batch=0), dict(_profile=[])

# model name -> constructor overrides (args of make_args; "table" = table dtype)
MODELS = {
    "main": {}, "bf16": dict(table="bf16"),
    "ho_only": dict(ablation="ho_only"), "ps_only": dict(ablation="ps_only"), "ho_only_uo_kg_eh": dict(ablation="ho_only_uo_kg_eh"),
    "no_ps_o_ft": dict(ablation="no_ps_o_ft"), "no_wd": dict(ablation="no_wd"),
    "h3": dict(h_hop=3), "h1": dict(h_hop=1), "p0": dict(p_hop=0), "nm68": dict(n_memory=68), "nm32": dict(n_memory=32),
    "nm6": dict(n_memory=6),
}

# every (schedule, feed, key_addressing) the grid reaches -- the recording must show exactly these
TRIPLES = sorted([
    ("small", "users", "users_feed"), ("small", "pairs", "per_pair"), ("small", "assembled", "per_pair"),
    ("native", "users", "flash"), ("native", "users", "gathered_er"), ("native", "users", "records"), ("native", "users", "grouped"),
    ("native", "users", "users_feed"), ("native", "pairs", "per_pair"), ("native", "assembled", "per_pair"),
    ("python", "users", "flash"), ("python", "users", "gathered_er"), ("python", "users", "records"), ("python", "users", "grouped"),
    ("python", "users", "users_feed"), ("python", "users", "none"), ("python", "pairs", "per_pair"), ("python", "pairs", "ripple"),
    ("python", "pairs", "none"), ("python", "assembled", "per_pair"), ("python", "assembled", "ripple"),
    ("python", "shared", "shared"), ("python", "shared", "none"),
])
# what route_plan.plan can return and the grid does not reach, with the reason: nothing (tests/test_route_plan_host.py enumerates
# the plan's inputs and finds no route outside the recorded ones)
UNREACHED = {}


def cases_of(name):
    """(group, attributes, feed, B, distinct_users, want_probs) of one model.  feed: uts (int32, contiguous, int64 user ids) |
    uts_nc (non-contiguous) | uts_i64 | uts_u32 (int32 user ids) | uts_one (a single user id) | pairs | shared | shared_one."""
    c = []
    if name == "main":
        # small_max_batch: the single launch up to 1 024 pairs, the native call beyond
        c += [("small_max", {}, f, B, None, False) for f in ("uts", "pairs") for B in (1024, 1025)]
        # native_l2_max_batch: per-pair lists and the ungrouped users feed fall to the Python schedule above 65 536; grouped never
        c += [("native_max", {}, "pairs", B, None, False) for B in (65536, 65537)]
        c += [("native_max_users", dict(group_min_pairs_per_user=4096), "uts", B, None, False) for B in (65536, 65537)]
        c += [("native_max_grouped", {}, "uts", 65537, None, False)]
        for sched in (SMALL_OFF, PROFILE):                     # the native call / the Python schedule
            # group_min_pairs_per_user: grouped from 4 pairs per user, of n_user or of the distinct_users hint
            c += [("grouped", sched, "uts", B, None, False) for B in (4 * N_USER - 1, 4 * N_USER)]
            c += [("grouped_hint", sched, "uts", B, 20, False) for B in (79, 80)]
            # the automatic flash rule: users x P x Nm >= nR x n_entity, 15 x 32 >= 480
            c += [("flash_hint", sched, "uts", 2048, d, False) for d in (14, 15, None)]
            c += [("flash_by_B", dict(sched, group_min_pairs_per_user=1), "uts", B, None, False) for B in (14, 15)]
            # MVIN.ka_flash / .ka_er / .static_user_records
            c += [("ka_flash=%s" % v, dict(sched, ka_flash=v), "uts", 2048, d, False) for v in (True, False) for d in (14, None)]
            c += [("ka_er", dict(sched, ka_er=True, ka_flash=f), "uts", 2048, None, False) for f in (False, None)]
            c += [("no_static", dict(sched, static_user_records=False), "uts", 2048, None, False)]
            # the feeds, ungrouped (100 pairs) and grouped (2 048)
            c += [("feeds", sched, f, B, None, False) for f in ("uts_nc", "uts_i64", "uts_u32", "pairs") for B in (100, 2048)]
        # the broadcast: a single user id for the batch
        c += [("broadcast", {}, f, B, None, False) for f in ("uts_one", "shared_one") for B in (1, 300)]
        c += [("broadcast", SMALL_OFF, "uts_one", 300, None, False)]
        c += [("feeds_small", {}, f, 100, None, False) for f in ("uts_nc", "uts_i64", "uts_u32", "pairs", "shared")]
        c += [("shared", {}, "shared", 2048, None, False)]
        # settings that rule the single launch and the native call out (or, validate_device_ids, do not)
        for nm, at in (("fused=False", dict(fused=False)), ("hoist", dict(hoist=True)), ("validate", dict(validate_device_ids=True)),
                       ("profile", PROFILE)):
            c += [(nm, at, f, B, None, False) for f in ("uts", "pairs") for B in (300, 2048)]
        c += [("fused=False", dict(fused=False), "uts_nc", 300, None, False)]
        c += [("want_probs", {}, f, B, None, True) for f in ("uts", "pairs") for B in (300, 2048)]
    elif name in ("bf16", "nm32"):
        # bf16: no single launch, no flash / gathered form, no records; nm32: a shape the records kernel takes
        for sched in ({}, SMALL_OFF, PROFILE):
            c += [("default", sched, f, B, None, False) for f in ("uts", "pairs") for B in (300, 2048)]
        for sched in (SMALL_OFF, PROFILE):
            c += [("ka_flash=%s" % v, dict(sched, ka_flash=v), "uts", 2048, None, False) for v in (True, False)]
            c += [("ka_er", dict(sched, ka_er=True, ka_flash=False), "uts", 2048, None, False)]
            c += [("no_static", dict(sched, static_user_records=False, ka_flash=False), "uts", 2048, None, False)]
    elif name == "nm6":
        # a shared list outside the dense form (Nm % 4 != 0) is replicated
        c += [("shared_replicated", {}, f, B, None, False) for f in ("shared", "shared_one") for B in (100, 2048)]
        c += [("default", {}, f, 300, None, False) for f in ("uts", "pairs")]
    else:
        # the wirings and shapes that take other schedules: h_hop = 3 rules out the native call, h_hop = 1 takes the single launch
        # only, Nm = 68 has no key-addressing kernel (the ripple_attn loop), the ablations without a preference set run none
        c += [("default", {}, f, B, None, False) for f in ("uts", "uts_u32", "pairs", "shared") for B in (100, 2048)]
        c += [("small_off", SMALL_OFF, f, 100, None, False) for f in ("uts", "pairs")]
    return c


def adjacency(K, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, N_ENTITY, (N_ENTITY, K), dtype=np.int64), rng.integers(0, N_RELATION, (N_ENTITY, K), dtype=np.int64)


class Built(object):
    """One model of the grid with its feeds and the mirror's outputs over the N_COMBOS distinct pairs (``want``) and over the same
    items scored for the first combo's user alone (``want_one``)."""

    def __init__(self, name):
        from oracle import mirror_fp32
        kw = dict(MODELS[name])
        table = kw.pop("table", "f32")
        self.args = make_args(**dict(SHAPE, batch_size=N_COMBOS, **kw))
        a = self.args
        seed = 77 + sorted(MODELS).index(name)
        adj_e, adj_r = adjacency(a.neighbor_sample_size, seed)
        params = init_params(a, N_USER, N_ENTITY, N_RELATION, seed=seed + 2, random_agg_bias=True)
        if table == "bf16":        # the kernels widen bf16 rows exactly: the mirror runs on the rounded table
            params = dict(params, entity_emb_matrix=torch.from_numpy(params["entity_emb_matrix"]).to(torch.bfloat16).float().numpy())
        self.model = MVIN(a, N_USER, N_ENTITY, N_RELATION, adj_e, adj_r, params=params, device="cuda:0", table_dtype=table)
        rng = np.random.default_rng(seed + 3)
        self.users, self.items = rng.integers(0, N_USER, N_COMBOS), rng.integers(0, N_ENTITY, N_COMBOS)
        self.uts_np = synth.ripple_sets(N_USER, N_ENTITY, N_RELATION, a.p_hop, a.n_memory, seed=seed + 4)
        dev = self.model.device
        self.uts = torch.from_numpy(self.uts_np).to(dev)
        wide = torch.zeros(self.uts.shape[:3] + (2 * a.n_memory,), dtype=torch.int32, device=dev)
        wide[..., ::2] = self.uts
        self.uts_nc, self.uts_i64 = wide[..., ::2], self.uts.long()
        self.want, self.want_one = {}, {}
        for want, users in ((self.want, self.users), (self.want_one, np.full(N_COMBOS, self.users[0]))):
            m = mirror_fp32.forward(a, params, adj_e, adj_r, users, self.items, *synth.memories_for(self.uts_np, users))
            want.update(scores=m.scores.numpy(), user_o=m.user_o.numpy(), item_embeddings=m.item_embeddings.numpy())

    def call(self, feed, B, distinct, want_probs):
        m, dev = self.model, self.model.device
        idx = np.arange(B) % N_COMBOS
        items = torch.from_numpy(self.items[idx]).to(dev)
        one = feed.endswith("_one")
        users_np = np.full(B, self.users[0]) if one or feed == "shared" else self.users[idx]
        users = torch.from_numpy(users_np[:1] if one else users_np).to(dev)
        if feed.startswith("uts"):
            uts = {"uts_nc": self.uts_nc, "uts_i64": self.uts_i64}.get(feed, self.uts)
            users = users.to(torch.int32) if feed == "uts_u32" else users
            out = m.forward_users(users, items, uts, want_probs=want_probs, distinct_users=distinct)
            return out, uts, None
        if feed == "pairs":
            mem = [[torch.from_numpy(x).to(dev) for x in lst] for lst in synth.memories_for(self.uts_np, users_np)]
        else:
            u0 = int(self.users[0])
            mem = [[self.uts[u0, i, x].contiguous() for i in range(self.uts.shape[1])] for x in range(3)]
        return m.forward_device(users, items, *mem, want_probs=want_probs), None, mem[0]

    def expected(self, feed, B):
        want = self.want_one if (feed.endswith("_one") or feed == "shared") else self.want
        idx = np.arange(B) % N_COMBOS
        return {k: v[idx] for k, v in want.items()}


def run_case(built, attrs, feed, B, distinct, want_probs):
    """One forward with the library's entry points wrapped -> (outcome dict, outputs)."""
    m = built.model
    for k, v in dict(BASE, **attrs).items():
        setattr(m, k, [] if k == "_profile" and v is not None else v)
    m._uts_records = None
    trace, native, saved, lib = [], [], {}, _lib.load()

    def wrap(name, fn):
        def traced(*a, **kw):
            tag = name + ("[records]" if kw.get("records") is not None else "") + ("[er]" if kw.get("er") is not None else "")
            if name == "key_addressing" and a[7].shape[0] == 1:       # the h-set read of ONE shared list (its output is one row)
                tag += "[one]"
            trace.append(tag)
            return fn(*a, **kw)
        return traced

    def wrap_native(name, fn):
        def traced(ref, *rest):
            native.append([name] + [p for p in ARG_POINTERS if getattr(ref._obj, p)])
            return fn(ref, *rest)
        return traced

    for name in TRACED:
        saved[name] = getattr(ops, name)
        setattr(ops, name, wrap(name, saved[name]))
    fns = {name: getattr(lib, name) for name in NATIVE}
    for name, fn in fns.items():
        setattr(lib, name, wrap_native(name, fn))
    m._small_state = m._native_l2_state = None            # (they hold the entry points they were built with)
    out = err = None
    try:
        out, uts, mem_h = built.call(feed, B, distinct, want_probs)
        torch.cuda.synchronize()
    except TypeError as e:                                # an int64 user_triplet_set: the per-pair kernel refuses the assembled lists
        err, uts, mem_h = str(e), built.uts_i64, None
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
        for name, fn in fns.items():
            setattr(lib, name, fn)
        m._small_state = m._native_l2_state = None
    oc = dict(trace=trace, native=native)
    if err is not None:
        oc["raises"] = err
    items = torch.zeros(B, dtype=torch.int64, device=m.device)
    m._distinct_hint = distinct                           # (the _ka_flash_for view reads the hint of the call at hand)
    views = dict(small=m._small_ok(items, mem_h, want_probs), small_static=m._small_static_ok(),
                 native_l2=m._native_l2_ok(items, mem_h, want_probs), native_l2_nocap=m._native_l2_ok(items, mem_h, want_probs, cap=False),
                 records_built=m._uts_records is not None and m._uts_records[3] is not None, flash_ws=bool(m._ka_flash_ws))
    if uts is not None:
        rec = m.user_records(uts)
        views.update(user_records=rec is not None, ka_flash=m._ka_flash_for(uts, rec, B), ka_er=m._ka_er_for(uts, rec),
                     ka_flash_norec=m._ka_flash_for(uts, None, B), ka_er_norec=m._ka_er_for(uts, None))
    oc["views"] = {k: bool(v) for k, v in views.items()}
    oc["route"] = observed_route(oc, feed, library_answers(m)["user_records"])
    m._ka_flash_ws.clear()
    m._profile = None
    return oc, out


def check_outputs(built, out, feed, B, what):
    for name, want in built.expected(feed, B).items():
        assert_close(getattr(out, name).cpu().numpy(), want, f"{name} vs fp32 mirror, {what}")


def library_answers(m):
    """The library's capability answers for the model's shape and table type."""
    D, K, P, Nm, nE, nR, set_ = m.dim, m.n_neighbor, m.p_hop, m.n_memory, m.n_entity, m.n_relation, bool(m.args.PS_O_ft)
    return dict(score_small=ops.score_small_supported(D, K, P, Nm, nR), l2_tail=ops.l2_tail_supported(D),
                gather_attn_l2=ops.gather_attn_l2_supported(D, K), key_addressing=ops.key_addressing_supported(Nm, D),
                key_addressing_grouped=ops.key_addressing_grouped_supported(D, P, Nm, nR),
                user_records=ops.user_records_supported(D, P, Nm, nR, m.table_dtype == "bf16"),
                key_addressing_flash=ops.key_addressing_flash_supported(D, P, Nm, nR, nE),
                key_addressing_grouped_er=ops.key_addressing_grouped_er_supported(D, P, Nm, nR, nE, set_),
                flash_tables_elems=int(_lib.load().mvin_key_addressing_flash_tables_elems(nE, nR, D, P, 1 if set_ else 0)),
                user_records_words=ops.user_records_len(P, Nm, nR))


def static_of(built):
    m = built.model
    E = m.entity_emb_matrix
    return dict(caps=library_answers(m), table_bytes=E.numel() * E.element_size(), adj_bytes=m.adj_entity.numel() * 4,
                n_user=N_USER, n_entity=N_ENTITY, n_relation=N_RELATION, dim=m.dim, K=m.n_neighbor, h_hop=m.h_hop, n_mix_hop=m.n_mix_hop,
                p_hop=m.p_hop, n_memory=m.n_memory, table_dtype=m.table_dtype,
                wiring={k: bool(getattr(m.args, k)) for k in ("wide_deep", "PS_only", "HO_only", "User_orient_kg_eh", "PS_O_ft")},
                # (the three batch thresholds: what every case sets, BASE -- the suite's fixtures build models with MVIN_SMALL=0)
                thresholds=dict(small_max_batch=BASE["small_max_batch"], native_l2_max_batch=BASE["native_l2_max_batch"],
                                group_min_pairs_per_user=BASE["group_min_pairs_per_user"], user_records_max_bytes=m.USER_RECORDS_MAX_BYTES,
                                flash_tables_max_bytes=m.FLASH_TABLES_MAX_BYTES))


def observed_route(oc, feed, records_kernel):
    """[schedule, feed, key_addressing] as the calls into the library show it."""
    tr, nat = oc["trace"], oc["native"]
    ka = ("flash" if "key_addressing_flash" in tr else
          "gathered_er" if "key_addressing_grouped[records][er]" in tr else
          "records" if "key_addressing_grouped[records]" in tr else "grouped" if "key_addressing_grouped" in tr else
          "users_feed" if "key_addressing_users" in tr else "shared" if ("row_softmax" in tr or "key_addressing[one]" in tr) else
          "per_pair" if "key_addressing" in tr else "ripple" if "ripple_attn" in tr else "none")
    if nat:
        args = nat[0][1:]
        sched = "small" if nat[0][0] == "mvin_score_small_fwd" else "native"
        fd = "users" if "uts" in args else "assembled" if feed.startswith("uts") else "pairs"
        # (the library takes the kernel over the records where it has one for the shape; else the pointer goes along unread)
        ka = ("per_pair" if "uts" not in args else "users_feed" if "group_ws" not in args else "flash" if "ka_flash" in args else
              "gathered_er" if "ka_er" in args else "records" if "user_records" in args and records_kernel else "grouped")
        return [sched, fd, ka]
    if feed.startswith("uts"):
        fd = "users" if ka in ("flash", "gathered_er", "records", "grouped", "users_feed", "none") else "assembled"
    else:
        fd = "shared" if (ka == "shared" or (ka == "none" and feed.startswith("shared"))) else "pairs"
    return ["python", fd, ka]


def record_model(name):
    """The recording of one model: its static inputs and, per case, the outcome."""
    built = Built(name)
    static, rows = static_of(built), []
    for group, attrs, feed, B, distinct, wp in cases_of(name):
        oc, out = run_case(built, attrs, feed, B, distinct, wp)
        if "raises" not in oc:
            check_outputs(built, out, feed, B, f"{name} {group} {feed} B={B}")
        rows.append(([group, {k: (v if k != "_profile" else True) for k, v in attrs.items()}, feed, B, distinct, wp], oc))
    return static, rows


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_routes_launches_and_outputs_are_the_recorded_ones(name, golden, hip_lib):
    g = golden["models"][name]
    built = Built(name)
    assert static_of(built) == g["static"]
    cases = cases_of(name)
    assert len(cases) == len(g["cases"]), "the grid is not the recorded one"
    replayed = 0
    for (group, attrs, feed, B, distinct, wp), c in zip(cases, g["cases"]):
        assert [group, {k: (v if k != "_profile" else True) for k, v in attrs.items()}, feed, B, distinct, wp] == c[:6], "the grid is not the recorded one"
        what = f"{name} {group} {attrs} {feed} B={B} distinct={distinct} want_probs={wp}"
        oc, out = run_case(built, attrs, feed, B, distinct, wp)
        want = golden["outcomes"][c[6]]
        for part in ("trace", "native", "views"):
            assert oc[part] == want[part], f"{part}, {what}: {oc[part]} != {want[part]}"
        assert oc.get("raises") == want.get("raises"), what
        if "raises" not in want:
            check_outputs(built, out, feed, B, what)
        replayed += 1
    assert replayed == len(g["cases"])


def test_the_recording_reaches_the_listed_routes(golden):
    seen = set()
    for g in golden["models"].values():
        for c in g["cases"]:
            seen.add(tuple(golden["outcomes"][c[6]]["route"]))
    assert sorted(seen) == TRIPLES
    assert not (set(UNREACHED) & seen)
