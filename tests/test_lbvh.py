"""The Morton-order builder (RT_BUILD_LBVH) on host-only scenes: the CPU statement of the tree the k_lbvh_*
kernels build (bvh.cpp build_lbvh), the builder selection entries, and the fallback to the SAH builder.

Scene S, the tiny scenes and the deformations are tests/_refit_scenes.py's. Equality is of bytes (digests).
"""
import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

import _refit_scenes as S

# info keys: triangles in leaves + always + never = all
def _covered(info):
    return info["leaf_triangles"] + info["always"] + info["never"]


@pytest.fixture(scope="module")
def arr(workdir):
    return S.base_arrays(workdir)


def _create(arr, vertices=None, builder="sah"):
    return R.Scene.create(arr["vertices"] if vertices is None else vertices, arr["triangles"], arr["tri_mat"],
                          arr["materials"], device=R.RT_HOST_ONLY, builder=builder)


def _tiny(name, builder):
    v, t, _ = S.tiny_scenes()[name]
    return R.Scene.create(v, t, np.zeros(len(t), np.uint32), S.TINY_MATERIALS, device=R.RT_HOST_ONLY, builder=builder)


def copies70():
    """70 copies of one triangle: every Morton code equal, so the whole tree comes from the tie-break."""
    v = np.tile(np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.1, 0.7, -0.2]], np.float32), (70, 1))
    t = np.arange(210, dtype=np.uint32).reshape(70, 3)
    return v, t


def test_builder_selection_round_trip(arr):
    with S.create(arr) as sc:
        assert sc.builder == ("sah", "sah")
        d0 = sc.bvh_digest()
        sc.set_builder("lbvh")
        assert sc.builder == ("lbvh", "sah")     # nothing is rebuilt
        assert sc.bvh_digest() == d0
        rc = _capi.lib().rt_scene_set_builder(sc.handle, 7)
        assert rc == _capi.RT_E_ARG
        assert sc.builder == ("lbvh", "sah") and sc.bvh_digest() == d0
        sc.set_builder("sah")
        assert sc.builder == ("sah", "sah")
        with pytest.raises(ValueError):
            sc.set_builder("ploc")
    # rt_scene_create is the SAH builder, as before: the same digest as create_ex(..., RT_BUILD_SAH)
    with S.create(arr) as a, _create(arr, builder="sah") as b:
        assert a.bvh_digest() == b.bvh_digest() and b.builder == ("sah", "sah")


def test_lbvh_tree_of_S(arr):
    with _create(arr, builder="lbvh") as sc, S.create(arr) as sah:
        sc.bvh_validate()
        assert sc.builder == ("lbvh", "lbvh")
        info, ref = sc.bvh_info(), sah.bvh_info()
        assert _covered(info) == len(arr["triangles"]) == 1642
        assert info["always"] == ref["always"] == 1 and info["never"] == ref["never"] == 1
        assert info["leaf_triangles"] == 1640
        assert 2 <= info["depth"] <= 40 and info["nodes4"] > 85
        print("S: lbvh", info, "sah", ref)
        assert sc.bvh_digest() != sah.bvh_digest()
        with _create(arr, builder="lbvh") as again:
            assert again.bvh_digest() == sc.bvh_digest()   # deterministic


def test_lbvh_tiny_scenes():
    with _tiny("one_triangle", "lbvh") as sc, _tiny("one_triangle", "sah") as sah:
        sc.bvh_validate()
        info = sc.bvh_info()
        assert sc.builder == ("lbvh", "lbvh")
        assert info["nodes"] == 1 and info["depth"] == 2 and info["leaf_triangles"] == 1 and info["nodes4"] == 1   # the root is a leaf
        assert info == sah.bvh_info()
    with _tiny("two_slivers", "lbvh") as sc, _tiny("two_slivers", "sah") as sah:
        sc.bvh_validate()
        info = sc.bvh_info()
        assert info["leaf_triangles"] == 0 and info["always"] == 2 and info["nodes"] == 1 and info["depth"] == 1   # the tree is empty
        assert info == sah.bvh_info()
        assert _covered(info) == 2


def test_coincident_triangles_use_the_tie_break():
    v, t = copies70()
    with R.Scene.create(v, t, np.zeros(70, np.uint32), S.TINY_MATERIALS, device=R.RT_HOST_ONLY, builder="lbvh") as sc:
        sc.bvh_validate()
        info = sc.bvh_info()
        assert sc.builder == ("lbvh", "lbvh")
        assert info["leaf_triangles"] == 70 and _covered(info) == 70
        assert info["depth"] == 7   # 70 equal codes split by position: ceil(log2(70 / 2)) = 6 inner levels + the leaves


def test_build_then_refit(arr):
    new = S.deform(arr["vertices"], 0.03)
    with _create(arr, builder="lbvh") as sc, _create(arr, new, builder="lbvh") as fresh:
        d0 = sc.bvh_digest()
        assert sc.update_vertices(new) == "refit"
        assert sc.builder == ("lbvh", "lbvh")
        sc.bvh_validate()
        # the refit keeps the first vertices' topology: it equals neither tree built from other vertices, and
        # a scene that builds from the deformed vertices and refits with the same ones keeps its own tree
        built = fresh.bvh_digest()
        assert fresh.update_vertices(new) == "refit"
        assert fresh.bvh_digest() == built
        refitted = sc.bvh_digest()
        assert refitted != d0 and refitted != built   # (986 nodes against 990: D(0.03) moves triangles across Morton cells)
        assert sc.update_vertices(arr["vertices"]) == "refit"
        assert sc.bvh_digest() == d0                  # and back: the first tree's bytes
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_lbvh"
        assert sc.bvh_digest() == built


@pytest.mark.parametrize("case", ["collapse", "squeeze"])
def test_class_change_rebuilds_with_lbvh(arr, case):
    new = getattr(S, case)(arr)
    with _create(arr, builder="lbvh") as sc, _create(arr, new, builder="lbvh") as fresh:
        sc.bvh_info()
        assert sc.update_vertices(new) == "rebuilt_lbvh"
        sc.bvh_validate()
        assert sc.bvh_digest() == fresh.bvh_digest()
        assert sc.builder == ("lbvh", "lbvh")


def test_set_builder_takes_effect_at_the_next_rebuild(arr):
    new = S.deform(arr["vertices"], 0.01)
    with S.create(arr) as sc, _create(arr, new, builder="lbvh") as lb, S.create(arr, new) as sah:
        sc.bvh_info()
        sc.set_builder("lbvh")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_lbvh"
        assert sc.builder == ("lbvh", "lbvh") and sc.bvh_digest() == lb.bvh_digest()
        sc.set_builder("sah")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt"
        assert sc.builder == ("sah", "sah") and sc.bvh_digest() == sah.bvh_digest()


def test_fallback_to_sah_when_too_deep(arr, monkeypatch):
    new = S.deform(arr["vertices"], 0.01)
    with _create(arr, builder="lbvh") as sc, S.create(arr, new) as sah:
        depth = sc.bvh_info()["depth"]
        assert depth > 12 and sc.builder == ("lbvh", "lbvh")
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", "12")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt"
        assert sc.builder == ("lbvh", "sah")
        assert sc.bvh_digest() == sah.bvh_digest()
        sc.bvh_validate()
        monkeypatch.delenv("RTAMD_LBVH_MAX_DEPTH")
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_lbvh"
        assert sc.builder == ("lbvh", "lbvh")
        # the bound is inclusive: a limit equal to the tree's depth still builds it
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", str(sc.bvh_info()["depth"]))
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt_lbvh"
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", str(sc.bvh_info()["depth"] - 1))
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt"
