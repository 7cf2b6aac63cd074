"""mvin_kg_field / mvin_kg_explore on the GPU against tests/explore_oracle.py: every bitmap word and every count must be equal
(everything is an integer; nothing may depend on the launch shape, the stream or what ran before)."""
import itertools

import numpy as np
import pytest

import explore_oracle as xo

pytestmark = pytest.mark.gpu

# the three synthetic shapes the exploration share was first measured on: (entities, mean degree, seed items, K)
SHAPES = {"e1500": (1500, 10.7, 200, 8), "e4000": (4000, 8.73, 1800, 4), "e3000": (3000, 30.0, 600, 8)}
N_REL = 6


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _case(name, seed=3):
    from mvin_amd import synth
    nE, deg, n_seed, K = SHAPES[name]
    kg = synth.synth_kg(nE, N_REL, deg, seed=seed)
    seeds = np.random.default_rng(seed).choice(nE, n_seed, replace=False)
    return kg, nE, seeds, K


def _device(kg, nE, seeds):
    import torch
    from mvin_amd import data_prep
    csr = data_prep.build_csr(kg, nE, device="cuda:0")
    index = data_prep.kg_edge_index(csr)
    return csr, index, torch.from_numpy(np.asarray(seeds, dtype=np.int32)).to("cuda:0")


def _dev_adj(adj_e, adj_r):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(adj_e, dtype=np.int32)).to("cuda:0"),
            torch.from_numpy(np.ascontiguousarray(adj_r, dtype=np.int32)).to("cuda:0"))


_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        kg, nE, seeds, K = _case(name)
        csr_np = xo.csr_of(kg, nE)
        _ORACLE[name] = (kg, nE, seeds, K, csr_np, xo.edges_by_head(*csr_np), xo.edge_index(*csr_np))
    return _ORACLE[name]


def _check_index(index, want):
    for got, exp in zip(index, want):
        assert np.array_equal(got.cpu().numpy(), exp)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_edge_index_is_distinct_and_sorted(hip_lib, name):
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle(name)
    _, index, _ = _device(kg, nE, seeds)
    _check_index(index, index_np)
    assert index[0].dtype.is_floating_point is False and index[1].dtype == index[2].dtype


@pytest.mark.parametrize("hops", [1, 2, 3, 4])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_field_matches_the_set_oracle(hip_lib, name, hops):
    import torch
    from mvin_amd import ops
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle(name)
    _, index, seeds_dev = _device(kg, nE, seeds)
    bits, counts = ops.kg_field(index, seeds_dev, hops)
    torch.cuda.synchronize()
    edges, sizes = xo.field(ebh, nE, seeds, hops)
    assert counts.cpu().tolist() == sizes + [len(edges)]
    assert np.array_equal(_u32(bits), xo.bits_of(edges, index_np))


@pytest.mark.parametrize("K", [1, 4, 8, 32])
@pytest.mark.parametrize("hops", [1, 2, 3, 4])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_explore_matches_the_set_oracle(hip_lib, name, hops, K):
    import torch
    from mvin_amd import data_prep, ops, synth
    kg, nE, seeds, _, csr_np, ebh, index_np = _oracle(name)
    csr, index, seeds_dev = _device(kg, nE, seeds)
    M = index_np[1].shape[0]
    explored = torch.zeros((M + 31) // 32, dtype=torch.int32, device="cuda:0")
    fld, _ = xo.field(ebh, nE, seeds, hops)
    # one adjacency from the numpy sampler, one from the HIP sampler: the accumulated set is their union
    a0 = synth.sample_adjacency(*synth.kg_to_csr(kg, nE), K, seed=11)
    a1 = tuple(t.cpu().numpy() for t in data_prep.construct_adj(csr, nE, K, seed=5))
    union = set()
    for adj_e, adj_r in (a0, a1):
        counts = ops.kg_explore(index, *_dev_adj(adj_e, adj_r), seeds_dev, hops, explored).cpu().tolist()
        got = xo.explore(ebh, nE, adj_e, adj_r, seeds, hops)
        assert got <= fld
        assert counts == [len(got), len(got - union), len(got | union)]
        union |= got
        assert np.array_equal(_u32(explored), xo.bits_of(union, index_np))


def test_full_adjacency_explores_the_whole_field(hip_lib):
    import torch
    from mvin_amd import ops
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle("e1500")
    _, index, seeds_dev = _device(kg, nE, seeds)
    for hops in (1, 2, 3):
        bits, counts = ops.kg_field(index, seeds_dev, hops)
        explored = torch.zeros_like(bits)
        c = ops.kg_explore(index, *_dev_adj(*xo.full_adjacency(index_np)), seeds_dev, hops, explored).cpu().tolist()
        assert c[0] == c[1] == c[2] == int(counts[-1]) and torch.equal(explored, bits)          # rate exactly 1


def test_hand_graph(hip_lib):
    import torch
    from mvin_amd import data_prep, ops
    kg, nE, seeds, exp = xo.hand_graph()
    csr = data_prep.build_csr(kg, nE, device="cuda:0")
    index = data_prep.kg_edge_index(csr)
    index_np = xo.edge_index(*xo.csr_of(kg, nE))
    _check_index(index, index_np)
    ebh = exp["by_head"]
    sd = torch.from_numpy(seeds.astype(np.int32)).to("cuda:0")        # a repeat, a degree-0 seed, 99 and -3 out of range
    for hops, (edges, sizes) in exp["field"].items():
        bits, counts = ops.kg_field(index, sd, hops)
        assert counts.cpu().tolist() == sizes + [len(edges)]
        assert np.array_equal(_u32(bits), xo.bits_of(edges, index_np))
    adj_e, adj_r = np.zeros((nE, 2), dtype=np.int64), np.zeros((nE, 2), dtype=np.int64)
    adj_e[0], adj_r[0] = [1, 1000], [0, 0]       # an id out of range
    adj_e[1], adj_r[1] = [2, 3], [1, 0]          # (1, 3, 0) is no edge: 3 is not followed
    adj_e[2], adj_r[2] = [3, 1], [0, 0]
    adj_e[3], adj_r[3] = [4, 4], [2, 2]
    adj_e[6], adj_r[6] = [-7, 2 ** 31 - 1], [-1, 5]
    for hops in (1, 2, 3, 4):
        explored = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        c = ops.kg_explore(index, *_dev_adj(adj_e, adj_r), sd, hops, explored).cpu().tolist()
        got = xo.explore(ebh, nE, adj_e, adj_r, seeds, hops)
        assert c == [len(got)] * 3 and np.array_equal(_u32(explored), xo.bits_of(got, index_np))
    only_dead = torch.tensor([5, 99, -3], dtype=torch.int32, device="cuda:0")
    bits, counts = ops.kg_field(index, only_dead, 3)
    assert counts.cpu().tolist() == [0, 0, 0, 0] and int(bits.abs().sum()) == 0


def test_no_seeds_and_no_triples(hip_lib):
    import torch
    from mvin_amd import data_prep, ops
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle("e1500")
    csr, index, seeds_dev = _device(kg, nE, seeds)
    none = torch.zeros(0, dtype=torch.int32, device="cuda:0")
    bits, counts = ops.kg_field(index, none, 2)
    assert counts.cpu().tolist() == [0, 0, 0] and int(bits.abs().sum()) == 0            # written in full: zeros
    adj = data_prep.construct_adj(csr, nE, 4, seed=1)
    explored = torch.zeros_like(bits)
    assert ops.kg_explore(index, *adj, none, 2, explored).cpu().tolist() == [0, 0, 0] and int(explored.abs().sum()) == 0
    # a KG without triples
    empty = data_prep.build_csr(np.zeros((0, 3), dtype=np.int64), 50, device="cuda:0")
    eidx = data_prep.kg_edge_index(empty)
    assert eidx[0].tolist() == [0] * 51 and eidx[1].numel() == 0
    s = torch.arange(10, dtype=torch.int32, device="cuda:0")
    bits, counts = ops.kg_field(eidx, s, 3)
    assert bits.numel() == 0 and counts.cpu().tolist() == [0, 0, 0, 0]
    z = data_prep.construct_adj(empty, 50, 4, seed=1)
    assert ops.kg_explore(eidx, *z, s, 3, bits.clone()).cpu().tolist() == [0, 0, 0]
    ex = data_prep.KGExploration(empty, np.arange(10), 2)
    assert ex.field_edges == 0 and ex.update(*z) == (0, 0, 0) and ex.rate == 0.0


def test_wrappers_refuse_bad_arguments(hip_lib):
    import torch
    from mvin_amd import _lib, ops
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle("e1500")
    _, index, seeds_dev = _device(kg, nE, seeds)
    for hops in (0, 9):
        with pytest.raises(_lib.MvinHipError, match="hops"):
            ops.kg_field(index, seeds_dev, hops)
    with pytest.raises(TypeError):
        ops.kg_field(index, seeds_dev.long(), 2)
    bits = torch.zeros((index[1].numel() + 31) // 32, dtype=torch.int32, device="cuda:0")
    adj = torch.zeros((nE, 4), dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError):
        ops.kg_explore(index, adj[:-1].contiguous(), adj[:-1].contiguous(), seeds_dev, 2, bits)
    with pytest.raises(ValueError):
        ops.kg_explore(index, adj, adj, seeds_dev, 2, bits[:-1].contiguous())
    with pytest.raises(_lib.MvinHipError):
        ops.kg_explore(index, adj.cpu(), adj, seeds_dev, 2, bits)


def test_hub_row_longer_than_65536_slots(hip_lib):
    import torch
    from mvin_amd import data_prep, ops
    rng = np.random.default_rng(5)
    hub_deg, nE = 70000, 70050
    spokes = np.arange(1, hub_deg + 1)
    kg = np.concatenate([np.stack([np.zeros(hub_deg, np.int64), spokes % 3, spokes], 1),
                         np.stack([rng.integers(1, nE, 5000), rng.integers(0, 3, 5000), rng.integers(1, nE, 5000)], 1)])
    seeds = np.array([0, 70049, 17])
    csr_np = xo.csr_of(kg, nE)
    ebh, index_np = xo.edges_by_head(*csr_np), xo.edge_index(*csr_np)
    assert int(np.diff(index_np[0]).max()) > 65536
    csr, index, seeds_dev = _device(kg, nE, seeds)
    _check_index(index, index_np)
    for hops in (1, 2, 3):
        bits, counts = ops.kg_field(index, seeds_dev, hops)
        edges, sizes = xo.field(ebh, nE, seeds, hops)
        assert counts.cpu().tolist() == sizes + [len(edges)] and np.array_equal(_u32(bits), xo.bits_of(edges, index_np))
    explored = torch.zeros_like(bits)
    union = set()
    for K, seed in ((8, 1), (32, 2)):
        adj = data_prep.construct_adj(csr, nE, K, seed=seed)
        c = ops.kg_explore(index, *adj, seeds_dev, 3, explored).cpu().tolist()
        got = xo.explore(ebh, nE, adj[0].cpu().numpy(), adj[1].cpu().numpy(), seeds, 3)
        assert c == [len(got), len(got - union), len(got | union)]
        union |= got
    assert np.array_equal(_u32(explored), xo.bits_of(union, index_np))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accumulation_over_six_adjacencies(hip_lib, name):
    """``new`` is the oracle's set difference, totals are monotone, and the accumulated bitmap does not depend on the order the
    six adjacencies are fed in; KGExploration reports the same numbers."""
    import torch
    from mvin_amd import data_prep, ops
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle(name)
    csr, index, seeds_dev = _device(kg, nE, seeds)
    hops = 2
    adjs = [data_prep.construct_adj(csr, nE, K, seed=2 + 2 * s) for s in range(6)]
    sets = [xo.explore(ebh, nE, a[0].cpu().numpy(), a[1].cpu().numpy(), seeds, hops) for a in adjs]
    fld, sizes = xo.field(ebh, nE, seeds, hops)
    ex = data_prep.KGExploration(csr, seeds, hops)
    assert ex.field_edges == len(fld) and ex.frontier_sizes == sizes
    union, last = set(), 0
    for a, got in zip(adjs, sets):
        now, new, total = ex.update(*a)
        assert (now, new, total) == (len(got), len(got - union), len(got | union)) and total >= last
        union |= got
        last = total
        assert ex.rate == total / len(fld) <= 1.0
    assert union <= fld
    want = xo.bits_of(union, index_np)
    assert np.array_equal(_u32(ex.explored_bits), want)
    for order in ([5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 4, 3]):
        explored = torch.zeros_like(ex.explored_bits)
        seen = set()
        for i in order:
            c = ops.kg_explore(index, *adjs[i], seeds_dev, hops, explored).cpu().tolist()
            assert c == [len(sets[i]), len(sets[i] - seen), len(sets[i] | seen)]
            seen |= sets[i]
        assert np.array_equal(_u32(explored), want)
    # numpy adjacencies, as MVIN.set_adjacency takes them
    ex2 = data_prep.KGExploration(csr, seeds, hops)
    assert ex2.update(adjs[0][0].cpu().numpy().astype(np.int64), adjs[0][1].cpu().numpy().astype(np.int64))[0] == len(sets[0])


def test_same_bits_again_after_other_work_and_under_another_launch_shape(hip_lib, monkeypatch):
    import torch
    from mvin_amd import data_prep, ops
    kg, nE, seeds, K, csr_np, ebh, index_np = _oracle("e3000")
    csr, index, seeds_dev = _device(kg, nE, seeds)
    adj = data_prep.construct_adj(csr, nE, K, seed=9)

    def run():
        bits, counts = ops.kg_field(index, seeds_dev, 3)
        explored = torch.zeros_like(bits)
        c = ops.kg_explore(index, *adj, seeds_dev, 3, explored)
        return bits.clone(), counts.clone(), explored, c.clone()

    first = run()
    again = run()
    x = torch.randn(2048, 2048, device="cuda:0")
    for _ in range(3):
        x = (x @ x).tanh()
    torch.cuda.synchronize()
    after = run()
    shaped = []
    for block, grid in (("64", "3"), ("1024", "1"), ("192", "1048576")):
        monkeypatch.setenv("MVIN_EXPLORE_BLOCK", block)
        monkeypatch.setenv("MVIN_EXPLORE_MAX_GRID", grid)
        shaped.append(run())
    monkeypatch.delenv("MVIN_EXPLORE_BLOCK")
    monkeypatch.delenv("MVIN_EXPLORE_MAX_GRID")
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # a non-default stream
        streamed = run()
    side.synchronize()
    for other in [again, after, streamed] + shaped:
        for a, b in zip(first, other):
            assert torch.equal(a, b)
    edges, sizes = xo.field(ebh, nE, seeds, 3)
    assert first[1].cpu().tolist() == sizes + [len(edges)] and np.array_equal(_u32(first[0]), xo.bits_of(edges, index_np))


def test_numpy_oracle_agrees_with_the_set_oracle_then_lastfm_shape(hip_lib):
    """The vectorised oracle is first held against the set oracle at the small shapes, then stands in for it at the
    last-fm_50core shape (930 k slots), where Python sets take too long."""
    import torch
    from mvin_amd import data_prep, ops, synth
    for name, hops in itertools.product(sorted(SHAPES), (1, 2, 3)):
        kg, nE, seeds, K, csr_np, ebh, index_np = _oracle(name)
        adj_e, adj_r = synth.sample_adjacency(*synth.kg_to_csr(kg, nE), K, seed=4)
        edges, sizes = xo.field(ebh, nE, seeds, hops)
        flags, np_sizes = xo.field_np(index_np, seeds, hops)
        assert np_sizes == sizes and np.array_equal(xo.pack_bits(flags), xo.bits_of(edges, index_np))
        assert np.array_equal(xo.pack_bits(xo.explore_np(index_np, adj_e, adj_r, seeds, hops)),
                              xo.bits_of(xo.explore(ebh, nE, adj_e, adj_r, seeds, hops), index_np))
    d = synth.DATASETS["last-fm_50core"]
    nE, K, hops = d["n_entity"], 8, 2
    kg = synth.synth_kg(nE, d["n_relation"], d["mean_degree"], seed=1, tail_exponent=d["tail_exponent"], head_sigma=d["head_sigma"])
    seeds = np.arange(0, d["n_item"], 3)
    csr, index, seeds_dev = _device(kg, nE, seeds)
    index_np = tuple(t.cpu().numpy() for t in index)
    # the index itself, checked by its definition: rows ascending and distinct by (dst, rel), the same edge set as the CSR
    row = np.repeat(np.arange(nE), np.diff(index_np[0]))
    key = (row * nE + index_np[1].astype(np.int64)) * d["n_relation"] + index_np[2]
    assert (np.diff(key) > 0).all()
    indptr, dst, rel = (t.cpu().numpy() for t in csr)
    raw = (np.repeat(np.arange(nE), np.diff(indptr)) * nE + dst.astype(np.int64)) * d["n_relation"] + rel
    assert np.array_equal(np.unique(raw), key)
    bits, counts = ops.kg_field(index, seeds_dev, hops)
    flags, sizes = xo.field_np(index_np, seeds, hops)
    assert counts.cpu().tolist() == sizes + [int(flags.sum())] and np.array_equal(_u32(bits), xo.pack_bits(flags))
    explored = torch.zeros_like(bits)
    acc = np.zeros_like(flags)
    for s in range(3):
        adj = data_prep.construct_adj(csr, nE, K, seed=2 + 2 * s)
        c = ops.kg_explore(index, *adj, seeds_dev, hops, explored).cpu().tolist()
        now = xo.explore_np(index_np, adj[0].cpu().numpy(), adj[1].cpu().numpy(), seeds, hops)
        assert c == [int(now.sum()), int((now & ~acc).sum()), int((now | acc).sum())]
        acc |= now
        assert not (acc & ~flags).any()
    assert np.array_equal(_u32(explored), xo.pack_bits(acc))
