"""The launch-shape rules of the ranking / MF heads and of the MF scorer and the lazy Adam, restated in plain Python for the tests.

``instance`` restates rank_head_shape() (mvin_amd/csrc/mvin_rank_head_body.h): which compiled (L2, NP) instance of
rank_head_kernel / mf_head_kernel a (G, D) selects, how many groups a workgroup takes and how wide a group's segment of phase 2 is.
``lanes_l2`` restates the L2 rule of launch_mf_scores / launch_sparse_adam_rows (mvin_amd/csrc/mvin_mf.hip).
tests/test_rank_head_shapes_host.py holds the GPU modules' shape lists to these rules, without a GPU.
"""
BLOCK = 256                                   # kRankBlock: threads of a workgroup, and kRankLds: score words in LDS
GS_LEGAL = range(1, 65)                       # G = 1 is the MF head's BCE
DS_LEGAL = range(4, 129, 4)

# every (L2, NP) the rule can return; each is one compiled instance of rank_head_kernel and one of mf_head_kernel
INSTANCES = frozenset({(0, 1), (1, 1), (2, 1), (3, 1), (3, 2), (4, 1), (4, 2), (4, 4), (5, 1), (5, 2), (5, 4), (5, 8)})
LANES_L2 = frozenset(range(6))                # the instances of mf_scores_kernel and of sparse_adam_rows_kernel


def lanes_l2(D):
    """log2 of the lanes per row: the power of two that covers D / 4 chunks of 16 bytes."""
    l2 = 0
    while (4 << l2) < D:
        l2 += 1
    return l2


def instance(G, D):
    """(L2, NP, ng, w_l2): lanes per row (log2), passes over a group's rows, groups per workgroup, segment width (log2)."""
    l2 = lanes_l2(D)
    w_l2 = 0 if G == 1 else 1
    while (1 << w_l2) < G:
        w_l2 += 1
    rpp = BLOCK >> l2                         # rows per pass
    np_, ng = 1, 1
    if G <= rpp:
        ng = rpp // G                         # whole groups that fit one pass
    else:
        while np_ * rpp < G:                  # one group, its rows in np passes
            np_ <<= 1
    return l2, np_, ng, w_l2


def phase2_trips(G, D):
    """Trips of phase 2's loop over a full workgroup's slots (ng segments of 2^w_l2 lanes, BLOCK lanes per trip)."""
    _, _, ng, w_l2 = instance(G, D)
    return ((ng << w_l2) + BLOCK - 1) // BLOCK


def idle_lanes(D):
    """Lanes of a row's lane group that hold no chunk of the row (chunk >= D / 4)."""
    return (1 << lanes_l2(D)) - D // 4


def pow2_group(G):
    """G is a power of two in 4..32: the segment of phase 2 is exactly G lanes wide, and more than one segment fits a wave."""
    return G in (4, 8, 16, 32)
