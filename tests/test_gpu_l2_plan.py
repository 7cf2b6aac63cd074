"""-m gpu: which kernel form the two deepest tree levels take, replayed against a recording.

tests/golden/l2_plan_cases.json holds, for a grid in which every selection rule flips once, what a forward launched (the ordered
``mvin_amd.ops`` calls of these levels and of key addressing), which optional pointers the native call's argument block carried,
and what every selection predicate of ``MVIN`` answered.  It was recorded with ``record_model`` below on the commit before the
selection moved into ``mvin_amd/l2_plan.py``; the replay asserts that nothing moved, and that every case's outputs agree with
the fp32 mirror of the reference graph.  The one case recorded after that commit is ``item_order_fallback`` (see FALLBACK)."""
import json
import os

import numpy as np
import pytest
import torch

from mvin_amd import ops, synth
from mvin_amd._lib import MvinHipError
from mvin_amd.config import make_args
from mvin_amd.model import MVIN
from mvin_amd.params import init_params

from parity import assert_close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l2_plan_cases.json")
N_ENTITY, N_RELATION, N_USER, P_HOP, N_MEMORY = 96, 5, 8, 2, 16
N_COMBOS = 96                          # distinct (user, item) pairs: batch row b holds combo b % N_COMBOS, the mirror runs once over them

TRACED = ("fold_tables", "score_l2_folded", "project_tables", "entity_aggregates", "gather_attn_l2_agg", "gather_attn_l2_prj",
          "gather_attn_l2_enc", "gather_attn_l2", "order_by_key", "l2_tail", "key_addressing_flash_prepare", "key_addressing_flash",
          "key_addressing_grouped", "project_relations")
ARG_POINTERS = ("enc_entity", "prj_tables", "agg_tables", "fold_ws", "fold_gather", "item_order_ws", "ka_flash", "ka_er", "user_records")

# (dim, fan-out, h_hop); n_mix_hop = 1
SHAPES = [(64, 16, 2), (64, 32, 2), (64, 64, 2), (32, 8, 2), (32, 16, 2), (32, 32, 2), (16, 8, 2), (128, 16, 2), (32, 8, 3), (64, 16, 3)]
VARIANT_SHAPES = [(64, 32, 2), (32, 16, 2)]            # a bf16 table and User_orient = 0, once each
BASE = dict(prj=None, agg=None, fold=None, dedup=None, item_order=None, ka_flash=None, ka_er=False)
OVERRIDES = [("default", {}), ("agg=False", dict(agg=False)), ("fold=False", dict(fold=False)), ("prj=False", dict(prj=False)),
             ("prj=True", dict(prj=True)), ("dedup=False", dict(dedup=False)), ("dedup=True", dict(dedup=True)),
             ("item_order=True", dict(item_order=True))]
KA_OVERRIDES = [("ka_flash=True", dict(ka_flash=True)), ("ka_flash=False", dict(ka_flash=False)), ("ka_er=True", dict(ka_er=True))]


# The one case whose outcome is NOT the earlier commit's: there the Python schedule passed a parent order that the library refused
# (MvinHipError, -3) because its wave-per-parent kernel does not apply; now the library drops the order, as mvin_score_l2_fwd always
# did.  1 601 relations: the first count whose two logit tables no longer fit that kernel's LDS at K = 16 (tests/test_gpu_prj.py).
FALLBACK = dict(key=(64, 16, 2, "repeats", "f32"), n_relation=1601, B=64, sched="python", feed="users",
                attrs=dict(dedup=True, prj=True, agg=False, fold=False, item_order=True))


def model_keys():
    keys = [(D, K, H, adj, "f32") for (D, K, H) in SHAPES for adj in ("repeats", "distinct")]
    keys += [(D, K, H, adj, var) for (D, K, H) in VARIANT_SHAPES for var in ("bf16", "no_uo") for adj in ("repeats", "distinct")]
    return keys


def key_name(key):
    return "D%dK%dH%d-%s-%s" % key


def batch_sizes(D, K, H):
    """Just below and at every threshold that applies to the shape (B values that flip nothing for a shape are left out)."""
    ppp = K ** (H - 2)                                   # level-(L-2) nodes per pair
    at = {-(-f * N_ENTITY // (K * ppp)) for f in (5, 10, 16)}                  # the projected-tables factors
    at.add(-(-2048 // ppp))                                                      # ENC_AUTO_MIN_PARENTS
    at.add(4 * N_USER)                                                           # pairs grouped by user
    if D == 64 and K <= 32 and H == 2:
        at.add(32768)                                                            # ITEM_ORDER_MIN_BATCH
    return sorted({b for t in at for b in (t - 1, t) if b >= 1})


def cases_of(key):
    """(override name, attributes, B, schedule, feed) of one model."""
    D, K, H, _, var = key
    out = []
    for sched in ("native", "python"):
        for name, attrs in OVERRIDES:
            out += [(name, attrs, B, sched, "users") for B in batch_sizes(D, K, H)]
        for name, attrs in KA_OVERRIDES:
            out += [(name, attrs, B, sched, "users") for B in (4 * N_USER - 1, 4 * N_USER, 2048)]
        if (D, K, H, var) == (64, 32, 2, "f32"):
            out += [("default", {}, B, sched, "pairs") for B in batch_sizes(D, K, H)]
    return out


def adjacency(kind, K, seed, n_relation=N_RELATION):
    """``repeats``: rows sampled with replacement from fewer than K edges (distinct fraction well under 0.75);
    ``distinct``: K distinct neighbours per row (fraction 1.0)."""
    rng = np.random.default_rng(seed)
    adj_e = np.zeros((N_ENTITY, K), dtype=np.int64)
    adj_r = rng.integers(0, n_relation, (N_ENTITY, K), dtype=np.int64)
    for x in range(N_ENTITY):
        if kind == "distinct":
            adj_e[x] = rng.permutation(N_ENTITY)[:K]
        else:
            deg = int(rng.integers(1, K // 2 + 1))
            ne, nr = rng.integers(0, N_ENTITY, deg), rng.integers(0, n_relation, deg)
            pick = rng.integers(0, deg, K)
            adj_e[x], adj_r[x] = ne[pick], nr[pick]
    return adj_e, adj_r


class Built(object):
    """One model of the grid with its feeds and the mirror's outputs over the N_COMBOS distinct pairs."""

    def __init__(self, key, n_relation=N_RELATION):
        from oracle import mirror_fp32
        D, K, H, adj, var = key
        nR = n_relation
        seed = 1000 * D + 10 * K + H
        kw = dict(dim=D, neighbor_sample_size=K, h_hop=H, n_mix_hop=1, p_hop=P_HOP, n_memory=N_MEMORY, batch_size=N_COMBOS)
        self.args = make_args(ablation="no_uo", **kw) if var == "no_uo" else make_args(**kw)
        adj_e, adj_r = adjacency(adj, K, seed + (adj == "distinct"), nR)
        params = init_params(self.args, N_USER, N_ENTITY, nR, seed=seed + 2, random_agg_bias=True)
        if var == "bf16":          # the kernels widen bf16 rows exactly: the mirror runs on the rounded table
            params = dict(params, entity_emb_matrix=torch.from_numpy(params["entity_emb_matrix"]).to(torch.bfloat16).float().numpy())
        self.model = MVIN(self.args, N_USER, N_ENTITY, nR, adj_e, adj_r, params=params, device="cuda:0",
                          table_dtype="bf16" if var == "bf16" else "f32")
        rng = np.random.default_rng(seed + 3)
        self.users, self.items = rng.integers(0, N_USER, N_COMBOS), rng.integers(0, N_ENTITY, N_COMBOS)
        self.uts_np = synth.ripple_sets(N_USER, N_ENTITY, nR, P_HOP, N_MEMORY, seed=seed + 4)
        self.uts = torch.from_numpy(self.uts_np).to(self.model.device)
        mh, mr, mt = synth.memories_for(self.uts_np, self.users)
        m = mirror_fp32.forward(self.args, params, adj_e, adj_r, self.users, self.items, mh, mr, mt)
        self.want = dict(scores=m.scores.numpy(), user_o=m.user_o.numpy(), item_embeddings=m.item_embeddings.numpy())
        self._feeds = {}

    def feed(self, B):
        f = self._feeds.get(B)
        if f is None:
            dev = self.model.device
            idx = np.arange(B) % N_COMBOS
            users, items = self.users[idx], self.items[idx]
            f = self._feeds[B] = (idx, torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev))
        return f

    def memories(self, B):
        """The per-pair feed of the same batch (train.py:117-120)."""
        users = self.users[np.arange(B) % N_COMBOS]
        return [[torch.from_numpy(x).to(self.model.device) for x in lst] for lst in synth.memories_for(self.uts_np, users)]

    def static(self):
        """What the selection reads of the model, as values."""
        m = self.model
        D, K = m.dim, m.n_neighbor
        enc = m.encoded_adjacency() if m.fused is not False else None
        return dict(dim=D, K=K, depth=m.n_mix_hop * m.h_hop, n_entity=m.n_entity, n_relation=m.n_relation, n_user=N_USER,
                    table_dtype=m.table_dtype, user_orient=bool(m.args.User_orient), fused=bool(m.fused),
                    distinct_fraction=None if enc is None else enc[3],
                    caps=dict(prj_plain=ops.gather_attn_l2_prj_supported(D, K, False, m.n_entity, m.n_relation),
                              agg=ops.gather_attn_l2_agg_supported(D, K, m.n_entity, m.n_relation),
                              fold=ops.score_l2_folded_supported(D, K, m.n_entity, m.n_relation),
                              fold_gather=ops.score_l2_folded_gather_supported(D, K, m.n_entity, m.n_relation),
                              enc=ops.encode_adjacency_supported(D, K)),
                    l2_supported=ops.gather_attn_l2_supported(D, K), tail_supported=ops.l2_tail_supported(D))


def run_case(built, attrs, B, sched, feed):
    """One forward with the traced callables wrapped -> (outcome dict, outputs or None)."""
    m = built.model
    for k, v in dict(BASE, **attrs).items():
        setattr(m, k, v)
    m._profile = [] if sched == "python" else None
    m._native_l2_state = None
    idx, users, items = built.feed(B)
    mem = built.memories(B) if feed == "pairs" else None
    trace, saved = [], {}

    def wrap(name, fn):
        def traced(*a, **kw):
            tag = name
            if name == "gather_attn_l2_prj" and kw.get("encoded", True) is False:
                tag += "[plain]"
            if kw.get("order") is not None:
                tag += "[order]"
            trace.append(tag)
            return fn(*a, **kw)
        return traced

    for name in TRACED:
        saved[name] = getattr(ops, name)
        setattr(ops, name, wrap(name, saved[name]))
    out = err = None
    try:
        if feed == "users":
            out = m.forward_users(users, items, built.uts)
        else:
            out = m.forward_device(users, items, *mem)
        torch.cuda.synchronize()
    except MvinHipError as e:
        err = str(e)
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    oc = dict(trace=trace)
    if err is not None:
        oc["raises"] = int(err.split("rc=")[1].split(")")[0])
    st = m._native_l2_state
    oc["native_args"] = None if st is None else [p for p in ARG_POINTERS if getattr(st["args"], p)]
    L, K = m.n_mix_hop * m.h_hop, m.n_neighbor
    n_parents = B if st is not None else B * K ** (L - 2)
    enc = m._enc_for_l2(False, n_parents)
    rec = m.user_records(built.uts)
    oc["facades"] = dict(
        enc=enc is not None, prj=m._prj_for_l2(B, n_parents), prj_plain=m._prj_plain_ok(), agg=m._agg_for(enc), fold=m._fold_for(enc),
        fold_gather=m._fold_gather_ok(), fold_shape=m._fold_shape_ok(), agg_shape=m._agg_shape_ok(), item_order=m._item_order_for(B),
        ka_flash=m._ka_flash_for(built.uts, rec, B), ka_er=m._ka_er_for(built.uts, rec),
        native_l2=m._native_l2_ok(items, None, False), small=m._small_ok(items, None, False))
    oc["facades"] = {k: bool(v) for k, v in oc["facades"].items()}
    oc["plan"] = observed_plan(oc)
    m._profile = None
    return oc, out


def observed_plan(oc):
    """[adjacency, form, item_order] as the launches / the argument block show it (None: the call raised before them)."""
    na, tr = oc["native_args"], oc["trace"]
    if na is not None:
        form = ("folded_gather" if "fold_gather" in na else "folded" if "fold_ws" in na else "aggregates" if "agg_tables" in na
                else "tables" if "prj_tables" in na else "unprojected")
        return ["encoded" if "enc_entity" in na else "plain", form, "item_order_ws" in na]
    io = "order_by_key" in tr
    for t in tr:
        if t == "fold_tables":
            return ["encoded", "folded", io]
        if t == "entity_aggregates":
            return ["encoded", "aggregates", io]
        if t.startswith("gather_attn_l2_prj"):
            return ["plain" if "[plain]" in t else "encoded", "tables", io]
        if t == "gather_attn_l2_enc":
            return ["encoded", "unprojected", io]
        if t == "gather_attn_l2":
            return ["plain", "unprojected", io]
    return None


def check_outputs(built, out, B, what):
    idx = built.feed(B)[0]
    for name, want in built.want.items():
        assert_close(getattr(out, name).cpu().numpy(), want[idx], f"{name} vs fp32 mirror, {what}")


def record_model(key):
    """The recording of one model: its static inputs and, per case, the outcome (an index into the list of distinct outcomes)."""
    built = Built(key)
    rows, worst = [], 0.0
    for name, attrs, B, sched, feed in cases_of(key):
        oc, out = run_case(built, attrs, B, sched, feed)
        if out is not None:
            idx = built.feed(B)[0]
            for nm, want in built.want.items():
                got = getattr(out, nm).cpu().numpy().astype(np.float64)
                worst = max(worst, float((np.abs(got - want[idx]) / (1e-5 * np.abs(want[idx]) + 1e-6)).max()))
        rows.append((name, B, sched, feed, oc))
    return built.static(), rows, worst


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("key", model_keys(), ids=key_name)
def test_forms_launches_and_outputs_are_the_recorded_ones(key, golden, hip_lib):
    g = golden["models"][key_name(key)]
    built = Built(key)
    assert built.static() == g["static"]
    cases = cases_of(key)
    assert [[n, B, s, f] for n, _, B, s, f in cases] == [c[:4] for c in g["cases"]], "the grid is not the recorded one"
    for (name, attrs, B, sched, feed), c in zip(cases, g["cases"]):
        what = f"{key_name(key)} {name} B={B} {sched} {feed}"
        oc, out = run_case(built, attrs, B, sched, feed)
        want = golden["outcomes"][c[4]]
        for part in ("trace", "native_args", "facades", "plan"):
            assert oc[part] == want[part], f"{part}, {what}: {oc[part]} != {want[part]}"
        assert oc.get("raises") == want.get("raises"), what
        if out is not None:
            check_outputs(built, out, B, what)


def test_item_order_fallback_case(golden, hip_lib):
    g = golden["item_order_fallback"]
    built = Built(FALLBACK["key"], n_relation=FALLBACK["n_relation"])
    assert built.static() == g["static"] and g["B"] == FALLBACK["B"]
    oc, out = run_case(built, FALLBACK["attrs"], FALLBACK["B"], FALLBACK["sched"], FALLBACK["feed"])
    assert oc == g["outcome"] and "raises" not in oc and "gather_attn_l2_prj[order]" in oc["trace"]
    check_outputs(built, out, FALLBACK["B"], "item-order fallback case")
    _, plain = run_case(built, dict(FALLBACK["attrs"], item_order=False), FALLBACK["B"], FALLBACK["sched"], FALLBACK["feed"])
    assert torch.equal(out.scores, plain.scores)
