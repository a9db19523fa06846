"""The agglomerative builder (RT_BUILD_CLUSTER) on host-only scenes: the CPU statement of the tree the
k_cluster_* kernels build (bvh.cpp build_cluster), the selection entries, rt_scene_build_info and the
fallback to the Morton builder.

Scene S, the tiny scenes and the deformations are tests/_refit_scenes.py's, the tie scenes
tests/_lbvh_scenes.py's. Equality is of bytes (digests).
"""
import math

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

import _lbvh_scenes as L
import _refit_scenes as S


def _covered(info):
    return info["leaf_triangles"] + info["always"] + info["never"]


@pytest.fixture(scope="module")
def arr(workdir):
    return S.base_arrays(workdir)


def _create(arr, vertices=None, builder="cluster"):
    return R.Scene.create(arr["vertices"] if vertices is None else vertices, arr["triangles"], arr["tri_mat"],
                          arr["materials"], device=R.RT_HOST_ONLY, builder=builder)


def _tiny(name, builder):
    v, t, _ = S.tiny_scenes()[name]
    return R.Scene.create(v, t, np.zeros(len(t), np.uint32), S.TINY_MATERIALS, device=R.RT_HOST_ONLY, builder=builder)


def test_builder_selection_round_trip(arr):
    assert _capi.BUILD_CLUSTER == 2 and _capi.UPDATED_REBUILT_CLUSTER == 3
    with S.create(arr) as sc:
        d0 = sc.bvh_digest()
        sc.set_builder("cluster")
        assert sc.builder == ("cluster", "sah")     # nothing is rebuilt
        assert sc.bvh_digest() == d0
        assert _capi.lib().rt_scene_set_builder(sc.handle, 7) == _capi.RT_E_ARG
        assert sc.builder == ("cluster", "sah") and sc.bvh_digest() == d0
        assert _capi.lib().rt_scene_set_builder(sc.handle, _capi.BUILD_CLUSTER) == 0
        sc.set_builder("sah")
        assert sc.builder == ("sah", "sah")
    with _create(arr) as sc:
        sc.bvh_info()   # (a host-only scene builds its trees when they are first asked for)
        assert sc.builder == ("cluster", "cluster")
    # rt_scene_create is the SAH builder, as before
    with S.create(arr) as a, _create(arr, builder="sah") as b:
        assert a.bvh_digest() == b.bvh_digest() and a.builder == ("sah", "sah")
        assert a.build_info()["built_with"] == "sah" and a.build_info()["iterations"] == 0


def test_cluster_tree_of_S(arr):
    with _create(arr) as sc, _create(arr, builder="lbvh") as lb, S.create(arr) as sah:
        sc.bvh_validate()
        info, ref = sc.bvh_info(), lb.bvh_info()
        assert _covered(info) == len(arr["triangles"]) == 1642
        assert info["always"] == ref["always"] == 1 and info["never"] == ref["never"] == 1
        assert info["leaf_triangles"] == 1640
        assert 2 <= info["depth"] <= 40
        # the leaf order is the Morton builder's: only the topology above it differs
        assert np.array_equal(sc.bvh_order()[0], lb.bvh_order()[0]) and np.array_equal(sc.bvh_order()[1], lb.bvh_order()[1])
        assert len({sc.bvh_digest(), lb.bvh_digest(), sah.bvh_digest()}) == 3
        bi = sc.build_info()
        print("S: cluster", info, bi, "lbvh", lb.build_info()["cost"], "sah", sah.build_info()["cost"])
        assert bi["built_with"] == "cluster" and bi["fallback"] == "none"
        assert 1 <= bi["iterations"] <= bi["max_iterations"] and 8 <= bi["radius"] <= 16
        with _create(arr) as again:
            assert again.bvh_digest() == sc.bvh_digest()   # deterministic


def test_cluster_tiny_scenes():
    with _tiny("one_triangle", "cluster") as sc, _tiny("one_triangle", "sah") as sah:
        sc.bvh_validate()
        assert sc.builder == ("cluster", "cluster")
        assert sc.bvh_info() == sah.bvh_info() and sc.bvh_info()["nodes"] == 1   # the root is a leaf
        assert sc.build_info()["iterations"] == 0 and sc.build_info()["cost"] == 1.0
    with _tiny("two_slivers", "cluster") as sc, _tiny("two_slivers", "sah") as sah:
        sc.bvh_validate()
        assert sc.bvh_info() == sah.bvh_info() and _covered(sc.bvh_info()) == 2   # the tree is empty
        assert sc.build_info()["cost"] == 0.0


def _tie_and_size_scenes(workdir):
    v70 = np.tile(np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.1, 0.7, -0.2]], np.float32), (70, 1))
    return {"copies70": (v70, np.arange(210, dtype=np.uint32).reshape(70, 3)),
            "soup": L.soup(700, 11, always=0.06, never=0.05), "copies": L.copies(300), "lattice": L.lattice(3000),
            "indexed_grid": L.indexed_grid(workdir)}


@pytest.mark.parametrize("name", ["copies70", "soup", "copies", "lattice", "indexed_grid"])
def test_cluster_validates_and_keeps_the_morton_order(workdir, name):
    v, t = _tie_and_size_scenes(workdir)[name]
    with L.create(v, t, builder="cluster") as sc, L.create(v, t, builder="lbvh") as lb:
        sc.bvh_validate()
        assert sc.builder == ("cluster", "cluster")
        info = sc.bvh_info()
        assert _covered(info) == len(t)
        assert info["always"] == lb.bvh_info()["always"] and info["never"] == lb.bvh_info()["never"]
        assert np.array_equal(sc.bvh_order()[0], lb.bvh_order()[0])
        assert np.array_equal(sc.bvh_order()[1], lb.bvh_order()[1])
        assert np.all(np.diff(sc.bvh_order()[1].astype(np.int64)) > 0)   # the always list ascends


def test_build_then_refit(arr):
    new = S.deform(arr["vertices"], 0.03)
    with _create(arr) as sc, _create(arr, new) as fresh:
        d0 = sc.bvh_digest()
        assert sc.update_vertices(new) == "refit"
        assert sc.builder == ("cluster", "cluster")
        sc.bvh_validate()
        # a scene that builds from the deformed vertices and refits with the same ones keeps its own tree
        built = fresh.bvh_digest()
        assert fresh.update_vertices(new) == "refit"
        assert fresh.bvh_digest() == built
        assert sc.bvh_digest() != d0
        assert sc.update_vertices(arr["vertices"]) == "refit"
        assert sc.bvh_digest() == d0                  # and back: the first tree's bytes
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_cluster"
        assert sc.bvh_digest() == built


def test_refit_of_a_scene_that_keeps_its_topology():
    # scale and shift keep every nearest-neighbour decision's inputs in proportion only approximately, so the
    # claim is the refit's: the moved scene's refitted tree validates and moving back restores the bytes
    v, t = L.soup(700, 11, always=0.06, never=0.05)
    with L.create(v, t, builder="cluster") as sc:
        d0 = sc.bvh_digest()
        assert sc.update_vertices(L.move(v)) == "refit"
        sc.bvh_validate()
        assert sc.update_vertices(v) == "refit" and sc.bvh_digest() == d0


@pytest.mark.parametrize("case", ["collapse", "squeeze"])
def test_class_change_rebuilds_with_cluster(arr, case):
    new = getattr(S, case)(arr)
    with _create(arr) as sc, _create(arr, new) as fresh:
        sc.bvh_info()
        assert sc.update_vertices(new) == "rebuilt_cluster"
        sc.bvh_validate()
        assert sc.bvh_digest() == fresh.bvh_digest()
        assert sc.builder == ("cluster", "cluster")


def test_set_builder_takes_effect_at_the_next_rebuild(arr):
    new = S.deform(arr["vertices"], 0.01)
    with S.create(arr) as sc, _create(arr, new) as cl, _create(arr, new, builder="lbvh") as lb:
        sc.bvh_info()
        sc.set_builder("cluster")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_cluster"
        assert sc.builder == ("cluster", "cluster") and sc.bvh_digest() == cl.bvh_digest()
        sc.set_builder("lbvh")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_lbvh"
        assert sc.bvh_digest() == lb.bvh_digest() and sc.build_info()["iterations"] == 0


def test_fallback_when_too_deep(arr, monkeypatch):
    new = S.deform(arr["vertices"], 0.01)
    with _create(arr) as sc, S.create(arr, new) as sah:
        depth = sc.bvh_info()["depth"]
        assert depth > 4 and sc.build_info()["fallback"] == "none"
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", "4")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt"   # (the Morton tree is deeper than 4 too)
        assert sc.builder == ("cluster", "sah")
        bi = sc.build_info()
        assert bi["fallback"] == "depth" and bi["built_with"] == "sah" and bi["iterations"] == 0
        assert sc.bvh_digest() == sah.bvh_digest()
        sc.bvh_validate()
        monkeypatch.delenv("RTAMD_LBVH_MAX_DEPTH")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_cluster"
        assert sc.builder == ("cluster", "cluster") and sc.build_info()["fallback"] == "none"
        # the bound is inclusive: a limit equal to the tree's depth still builds it
        d = sc.bvh_info()["depth"]
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", str(d))
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_cluster"
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", str(d - 1))
        assert sc.update_vertices(new, mode="rebuild") != "rebuilt_cluster"
        assert sc.builder[1] != "cluster" and sc.build_info()["fallback"] == "depth"


def test_equal_boxes_halve_every_iteration():
    # 2,500 copies of one triangle: every distance is equal, so the key (distance, i XOR j) alone decides.
    # Buddies 2k, 2k + 1 pair up and the count halves: ceil(log2 2500) = 12 iterations. A "lowest index
    # wins" rule would merge one pair per iteration and need about 2,500. The cap allows for counts that
    # are odd on the way down (a leftover cluster waits one iteration), at most a couple.
    n = 2500
    v, t = L.copies(n)
    with L.create(v, t, builder="cluster") as sc:
        sc.bvh_validate()
        bi = sc.build_info()
        print("copies:", bi, sc.bvh_info())
        assert bi["built_with"] == "cluster"
        assert math.ceil(math.log2(n)) == 12 <= bi["iterations"] <= 14
        assert bi["iterations"] == 12   # what the halvings 2500 -> 1 take
        assert _covered(sc.bvh_info()) == n


def test_clustering_lowers_the_cost_of_the_grid(workdir):
    # The radix tree splits by code bits and ignores box size: the back plane's two big triangles inflate
    # its upper boxes. Unpadded-box prototype: radix 3.60, clustered 1.55 (ratio 0.43).
    v, t = L.indexed_grid(workdir)
    cost = {}
    for b in ("sah", "lbvh", "cluster"):
        with L.create(v, t, builder=b) as sc:
            cost[b] = sc.build_info()["cost"]
    print("indexed grid costs:", cost)
    assert cost["cluster"] < cost["lbvh"]
    assert all(c > 1.0 for c in cost.values())   # at least the root's two child boxes over their union
