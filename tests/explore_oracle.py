"""Oracle of the KG exploration counts (mvin_kg_field / mvin_kg_explore), written from the definitions with Python sets, plus a
vectorised numpy form of the same definitions for graphs too large for sets.  No GPU, no mvin_amd import.

Definitions (include/mvin_hip.h):
  * the KG is an undirected CSR (indptr, dst, rel); an EDGE is a distinct triple (h, t, r) with (t, r) listed under h;
  * field:    F_0 = seeds in range; for i < hops every edge with its head in F_i is in the field, F_{i+1} = their tails;
  * explored: G_0 = seeds in range; for i < hops, h in G_i, k < K: (h, adj_e[h,k], adj_r[h,k]) is explored when it is an edge,
              and only then its tail is in G_{i+1}.
"""
import numpy as np


def edges_by_head(indptr, dst, rel):
    """{h: set of (t, r)} -- duplicate slots of a row collapse."""
    indptr, dst, rel = (np.asarray(a) for a in (indptr, dst, rel))
    out = {}
    for h in range(indptr.shape[0] - 1):
        row = {(int(dst[e]), int(rel[e])) for e in range(int(indptr[h]), int(indptr[h + 1]))}
        if row:
            out[h] = row
    return out


def edge_index(indptr, dst, rel):
    """(eptr int64 [nE+1], edst int32 [M], erel int32 [M]): distinct (t, r) per row, ascending -- what
    data_prep.kg_edge_index must return."""
    ebh = edges_by_head(indptr, dst, rel)
    n_entity = np.asarray(indptr).shape[0] - 1
    eptr, edst, erel = np.zeros(n_entity + 1, dtype=np.int64), [], []
    for h in range(n_entity):
        for (t, r) in sorted(ebh.get(h, ())):
            edst.append(t)
            erel.append(r)
        eptr[h + 1] = len(edst)
    return eptr, np.asarray(edst, dtype=np.int32), np.asarray(erel, dtype=np.int32)


def field(ebh, n_entity, seeds, hops):
    """(set of (h, t, r), [|F_1|, ..., |F_hops|])."""
    front = {int(s) for s in seeds if 0 <= int(s) < n_entity}
    edges, sizes = set(), []
    for _ in range(hops):
        nxt = set()
        for h in front:
            for (t, r) in ebh.get(h, ()):
                edges.add((h, t, r))
                nxt.add(t)
        front = nxt
        sizes.append(len(front))
    return edges, sizes


def explore(ebh, n_entity, adj_e, adj_r, seeds, hops):
    """The set of (h, t, r) the adjacency explores."""
    adj_e, adj_r = np.asarray(adj_e), np.asarray(adj_r)
    front = {int(s) for s in seeds if 0 <= int(s) < n_entity}
    edges = set()
    for _ in range(hops):
        nxt = set()
        for h in front:
            row = ebh.get(h, ())
            for k in range(adj_e.shape[1]):
                t, r = int(adj_e[h, k]), int(adj_r[h, k])
                if (t, r) in row:
                    edges.add((h, t, r))
                    nxt.add(t)
        front = nxt
    return edges


def bits_of(edges, index):
    """The bitmap (uint32 [ceil(M/32)]) of a set of (h, t, r) over an ``edge_index`` triple: bit e = slot e."""
    eptr, edst, erel = index
    M = edst.shape[0]
    slot = {}
    for h in range(eptr.shape[0] - 1):
        for e in range(int(eptr[h]), int(eptr[h + 1])):
            slot[(h, int(edst[e]), int(erel[e]))] = e
    flags = np.zeros(((M + 31) // 32) * 32, dtype=bool)
    for edge in edges:
        flags[slot[edge]] = True
    return pack_bits(flags)


def pack_bits(flags):
    flags = np.asarray(flags, dtype=bool)
    pad = (-flags.shape[0]) % 32
    flags = np.concatenate([flags, np.zeros(pad, dtype=bool)])
    return (flags.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def popcount(bits):
    return int(np.unpackbits(np.ascontiguousarray(bits).view(np.uint8)).sum())


# --------------------------------------------------------------------------- the same definitions, vectorised
def field_np(index, seeds, hops):
    """(bool [M], [|F_1| ...]) over an edge index."""
    eptr, edst, erel = index
    n_entity = eptr.shape[0] - 1
    row = np.repeat(np.arange(n_entity), np.diff(eptr))
    seeds = np.asarray(seeds, dtype=np.int64)
    front = np.zeros(n_entity, dtype=bool)
    front[seeds[(seeds >= 0) & (seeds < n_entity)]] = True
    flags, sizes = np.zeros(edst.shape[0], dtype=bool), []
    for _ in range(hops):
        into = front[row]
        flags |= into
        front = np.zeros(n_entity, dtype=bool)
        front[edst[into]] = True
        sizes.append(int(front.sum()))
    return flags, sizes


def explore_np(index, adj_e, adj_r, seeds, hops):
    """bool [M]: the slots the adjacency explores."""
    eptr, edst, erel = index
    n_entity, M = eptr.shape[0] - 1, edst.shape[0]
    flags = np.zeros(M, dtype=bool)
    if M == 0:
        return flags
    adj_e, adj_r = np.asarray(adj_e, dtype=np.int64), np.asarray(adj_r, dtype=np.int64)
    n_rel = int(erel.max()) + 1
    row = np.repeat(np.arange(n_entity, dtype=np.int64), np.diff(eptr))
    keys = (row * n_entity + edst) * n_rel + erel                     # ascending: rows ascending by (dst, rel)
    seeds = np.asarray(seeds, dtype=np.int64)
    front = np.zeros(n_entity, dtype=bool)
    front[seeds[(seeds >= 0) & (seeds < n_entity)]] = True
    for _ in range(hops):
        h = np.flatnonzero(front)
        t, r = adj_e[h].reshape(-1), adj_r[h].reshape(-1)
        hh = np.repeat(h, adj_e.shape[1])
        ok = (t >= 0) & (t < n_entity) & (r >= 0) & (r < n_rel)
        q = (hh[ok] * n_entity + t[ok]) * n_rel + r[ok]
        pos = np.minimum(np.searchsorted(keys, q), M - 1)
        hit = keys[pos] == q
        flags[pos[hit]] = True
        front = np.zeros(n_entity, dtype=bool)
        front[t[ok][hit]] = True
    return flags


# --------------------------------------------------------------------------- a graph small enough to enumerate by hand
def hand_graph():
    """7 entities, triples (h, r, t):
         (0, 0, 1) twice   -- a duplicate triple
         (1, 1, 1)         -- a self-loop (listed under 1 twice by the undirected CSR: one edge)
         (1, 0, 2), (1, 1, 2) -- two relations between one pair
         (2, 0, 3), (3, 2, 4)
       entity 5 has no triples (a degree-0 seed), entity 6 neither; seeds = [0, 5, 99, -3, 0] (99 and -3 out of range).
    Returns (kg [n, 3], n_entity, seeds, expected) with the distinct undirected edges by head written out by hand."""
    kg = np.array([[0, 0, 1], [0, 0, 1], [1, 1, 1], [1, 0, 2], [1, 1, 2], [2, 0, 3], [3, 2, 4]], dtype=np.int64)
    by_head = {0: {(1, 0)},
               1: {(0, 0), (1, 1), (2, 0), (2, 1)},
               2: {(1, 0), (1, 1), (3, 0)},
               3: {(2, 0), (4, 2)},
               4: {(3, 2)}}
    # from seed 0: F_0 = {0}; level 0 edges (0,1,0), F_1 = {1}; level 1 edges (1,0,0) (1,1,1) (1,2,0) (1,2,1), F_2 = {0, 1, 2};
    # level 2 adds (2,1,0) (2,1,1) (2,3,0) (and repeats the others), F_3 = {0, 1, 2, 3}
    field_by_hops = {1: ({(0, 1, 0)}, [1]),
                     2: ({(0, 1, 0), (1, 0, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1)}, [1, 3]),
                     3: ({(0, 1, 0), (1, 0, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1), (2, 1, 0), (2, 1, 1), (2, 3, 0)}, [1, 3, 4])}
    return kg, 7, np.array([0, 5, 99, -3, 0], dtype=np.int64), {"by_head": by_head, "field": field_by_hops, "n_edges": 11}


def csr_of(kg, n_entity):
    """construct_kg as a CSR on the host (every triple under its head and under its tail, in file order)."""
    kg = np.asarray(kg, dtype=np.int64).reshape(-1, 3)
    src = np.stack([kg[:, 0], kg[:, 2]], 1).reshape(-1)
    dst = np.stack([kg[:, 2], kg[:, 0]], 1).reshape(-1)
    rel = np.stack([kg[:, 1], kg[:, 1]], 1).reshape(-1)
    order = np.argsort(src, kind="stable")
    indptr = np.zeros(n_entity + 1, dtype=np.int64)
    np.add.at(indptr, src + 1, 1)
    np.cumsum(indptr, out=indptr)
    return indptr, dst[order].astype(np.int32), rel[order].astype(np.int32)


def full_adjacency(index):
    """An adjacency that lists every edge of every row (K = the longest row; shorter rows repeat their first edge, rows
    without edges are zero rows): it must explore the whole field."""
    eptr, edst, erel = index
    n_entity = eptr.shape[0] - 1
    K = max(1, int(np.diff(eptr).max()) if n_entity else 1)
    adj_e, adj_r = np.zeros((n_entity, K), dtype=np.int64), np.zeros((n_entity, K), dtype=np.int64)
    for h in range(n_entity):
        a, b = int(eptr[h]), int(eptr[h + 1])
        if b > a:
            adj_e[h, :b - a], adj_r[h, :b - a] = edst[a:b], erel[a:b]
            adj_e[h, b - a:], adj_r[h, b - a:] = edst[a], erel[a]
    return adj_e, adj_r
