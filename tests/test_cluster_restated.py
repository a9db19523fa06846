"""A second statement of the agglomerative builder's clustering (RT_BUILD_CLUSTER on host-only scenes).

tests/test_cluster.py and the GPU tests compare the kernels with bvh.cpp's build_cluster, and both include
cluster_shared.h: a wrong window bound, key or leaf rule there would pass them all. The reference here is
NumPy and uses none of that text: the padded box per triangle from bvh_acceptance_box, the leaf order from
rt_scene_bvh_order, one cluster per leaf slot; every iteration the half-area dx dy + dy dz + dz dx of the
union box in float64 for every pair at most r positions apart, per cluster the minimum of (distance,
i XOR j), a merge of every mutual pair into the lower position (two single triangles in adjacent slots
become one leaf, everything else a node), and compaction in order. What it predicts: the node count and depth
of both trees (bvh_info fields 0, 1, 5, 6), the iteration count, and the tree cost of rt_scene_build_info.
"""
import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd.api import bvh_acceptance_box

import _lbvh_scenes as L
import _refit_scenes as S


def _half_area(lo, hi):
    e = hi.astype(np.float64) - lo.astype(np.float64)
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


def reference_clustering(lo, hi, r):
    """lo, hi: float32 (np, 3) boxes in leaf-slot order, np >= 3. Returns (nodes, depth, nodes4, depth4,
    iterations, cost)."""
    n = len(lo)
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and n >= 3
    # a cluster: ("leaf", first slot, count) or ("node", creation index)
    what = [("leaf", j, 1) for j in range(n)]
    made = []   # per node, in creation order: (child, child, lo0, hi0, lo1, hi1)
    iterations = 0
    while len(what) > 1:
        c = len(what)
        best = np.full(c, np.inf)
        best_x = np.full(c, np.iinfo(np.int64).max, np.int64)
        nn = np.full(c, -1, np.int64)
        for d in range(1, min(r, c - 1) + 1):
            i = np.arange(c - d, dtype=np.int64)
            j = i + d
            dist = _half_area(np.minimum(lo[:-d], lo[d:]), np.maximum(hi[:-d], hi[d:]))
            x = i ^ j
            for a, b in ((i, j), (j, i)):
                better = (dist < best[a]) | ((dist == best[a]) & (x < best_x[a]))
                best[a[better]], best_x[a[better]], nn[a[better]] = dist[better], x[better], b[better]
        assert (nn >= 0).all()
        mutual = nn[nn] == np.arange(c)
        assert mutual.any()   # the globally smallest key is mutual
        new_what, new_lo, new_hi = [], [], []
        for i in range(c):
            j = int(nn[i])
            if mutual[i] and j < i:
                continue   # the higher position dies
            if not mutual[i]:
                new_what.append(what[i]); new_lo.append(lo[i]); new_hi.append(hi[i])
                continue
            a, b = what[i], what[j]
            if a[0] == "leaf" and b[0] == "leaf" and a[2] == 1 and b[2] == 1 and b[1] == a[1] + 1:
                new_what.append(("leaf", a[1], 2))
            else:
                new_what.append(("node", len(made)))
                made.append((a, b, lo[i], hi[i], lo[j], hi[j]))
            new_lo.append(np.minimum(lo[i], lo[j])); new_hi.append(np.maximum(hi[i], hi[j]))
        what, lo, hi = new_what, np.array(new_lo, np.float32), np.array(new_hi, np.float32)
        iterations += 1
        assert iterations <= 10000
    assert what[0] == ("node", len(made) - 1)   # the root is the node made last
    depth = np.zeros(len(made), np.int64)
    for k in range(len(made) - 1, -1, -1):   # parents are made after their children
        for child in made[k][:2]:
            if child[0] == "node":
                assert child[1] < k
                depth[child[1]] = depth[k] + 1
    even = depth[depth % 2 == 0]
    # cost: node ids are the reverse of creation order
    total = 0.0
    for k in range(len(made) - 1, -1, -1):
        _, _, lo0, hi0, lo1, hi1 = made[k]
        total += float(_half_area(lo0, hi0))
        total += float(_half_area(lo1, hi1))
    _, _, lo0, hi0, lo1, hi1 = made[-1]
    root = float(_half_area(np.minimum(lo0, lo1), np.maximum(hi0, hi1)))
    return len(made), int(depth.max()) + 2, len(even), int(even.max()) // 2 + 1, iterations, total / root


def _boxes_in_leaf_order(v, t, leaf):
    lo, hi = np.zeros((len(leaf), 3), np.float32), np.zeros((len(leaf), 3), np.float32)
    for slot, tri in enumerate(leaf):
        st, a, b = bvh_acceptance_box(v[t[tri]])
        assert st == 0
        lo[slot], hi[slot] = a, b
    return lo, hi


def _scene(name, workdir):
    if name == "S":
        arr = S.base_arrays(workdir)
        return arr["vertices"], arr["triangles"]
    if name == "indexed_grid":
        return L.indexed_grid(workdir)
    if name == "soup":
        return L.soup(1500, 77, always=0.05, never=0.04)
    return L.lattice(3000)


@pytest.mark.parametrize("name", ["S", "indexed_grid", "soup", "lattice"])
def test_clustering_equals_the_numpy_statement(name, workdir):
    v, t = _scene(name, workdir)
    with L.create(v, t, builder="cluster") as sc:
        leaf, always = sc.bvh_order()
        info, bi = sc.bvh_info(), sc.build_info()
        assert sc.builder == ("cluster", "cluster")
    if name in ("S", "soup"):
        assert len(always) > 0 and info["never"] > 0   # fewer leaf slots than triangles
    lo, hi = _boxes_in_leaf_order(np.asarray(v, np.float32), t, leaf)
    nodes, depth, nodes4, depth4, iterations, cost = reference_clustering(lo, hi, bi["radius"])
    print(name, dict(nodes=nodes, depth=depth, nodes4=nodes4, depth4=depth4, iterations=iterations, cost=cost), info, bi)
    assert (info["nodes"], info["depth"], info["nodes4"], info["depth4"]) == (nodes, depth, nodes4, depth4)
    assert bi["iterations"] == iterations
    # the same sum in another association: at most 1e5 binary64 additions, each relative 1.1e-16
    assert abs(bi["cost"] - cost) <= 1e-9 * cost
