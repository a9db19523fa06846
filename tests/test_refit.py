"""Dynamic geometry on the host (rt_scene_update_vertices on host-only scenes, bvh.cpp refit_bvh): the CPU
statement of what the device refit kernels compute.

A refit keeps the tree's topology and recomputes every box as the exact min/max union of what lies below
it, so it validates whatever the deformation; it reproduces the builder's boxes when nothing moved (equal
digests); a triangle that changes class (in the tree / always tested / never accepted) forces a rebuild,
which gives the tree of a scene freshly created from the same arrays.
"""
import ctypes as C

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

import _refit_scenes as S


@pytest.fixture(scope="module")
def arr(workdir):
    return S.base_arrays(workdir)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_scene_s_has_every_class(arr):
    with S.create(arr) as sc:
        info = sc.bvh_info()
        assert info["always"] == 1 and info["never"] == 1 and info["leaf_triangles"] == 1640
        assert info["nodes4"] > 85   # past the breadth-first top levels
        sc.bvh_validate()


def test_oracle_reads_back_the_exact_vertices(arr, workdir):
    """The oracle frames of tests/test_gpu_refit.py come from OBJ files: the files hold these arrays' bits."""
    S.oracle_scene(arr, arr["vertices"], workdir, "refit_s")
    S.oracle_scene(arr, S.deform(arr["vertices"], 0.03), workdir, "refit_d003")


def test_refit_is_valid_and_keeps_topology(arr):
    new = S.deform(arr["vertices"], 0.03)
    with S.create(arr) as sc, S.create(arr, new) as fresh:
        info0, d0 = sc.bvh_info(), sc.bvh_digest()
        assert sc.update_vertices(new) == "refit"
        sc.bvh_validate()
        info1 = sc.bvh_info()
        assert {k: info1[k] for k in ("nodes", "nodes4", "always", "never", "leaf_triangles", "depth", "depth4")} == \
               {k: info0[k] for k in ("nodes", "nodes4", "always", "never", "leaf_triangles", "depth", "depth4")}
        assert sc.bvh_digest() != d0
        e, f = sc.export(), fresh.export()
        assert np.array_equal(_bits(e["vertices"]), _bits(new))
        assert np.array_equal(_bits(e["normals"]), _bits(f["normals"]))
        assert np.array_equal(e["triangles"], arr["triangles"]) and np.array_equal(e["tri_mat"], arr["tri_mat"])


def test_identity_update_reproduces_the_builders_boxes(arr):
    with S.create(arr) as sc:
        d0 = sc.bvh_digest()
        assert sc.update_vertices(arr["vertices"]) == "refit"
        assert sc.bvh_digest() == d0
        sc.bvh_validate()


def test_refit_back_gives_the_first_tree(arr):
    """Boxes are a function of topology and vertices alone: deforming and undoing restores every byte."""
    with S.create(arr) as sc:
        d0 = sc.bvh_digest()
        assert sc.update_vertices(S.deform(arr["vertices"], 0.03)) == "refit"
        assert sc.update_vertices(arr["vertices"]) == "refit"
        assert sc.bvh_digest() == d0


@pytest.mark.parametrize("case", ["collapse", "squeeze"])
def test_class_change_rebuilds(arr, case):
    new = getattr(S, case)(arr)
    with S.create(arr) as sc, S.create(arr, new) as fresh:
        sc.bvh_info()
        assert sc.update_vertices(new) == "rebuilt"
        sc.bvh_validate()
        assert sc.bvh_info() == fresh.bvh_info()
        assert sc.bvh_digest() == fresh.bvh_digest()
        assert np.array_equal(_bits(sc.export()["normals"]), _bits(fresh.export()["normals"]))


def test_rebuild_on_request_gives_the_fresh_tree(arr):
    new = S.deform(arr["vertices"], 0.03)
    with S.create(arr) as sc, S.create(arr, new) as fresh:
        assert sc.update_vertices(new, mode="rebuild") == "rebuilt"
        sc.bvh_validate()
        assert sc.bvh_digest() == fresh.bvh_digest()


def test_errors_leave_the_scene_untouched(arr):
    L = _capi.lib()
    v = np.ascontiguousarray(S.deform(arr["vertices"], 0.03))
    p = v.ctypes.data_as(C.c_void_p)
    n = len(v)
    with S.create(arr) as sc:
        d0, e0 = sc.bvh_digest(), sc.export()
        out = C.c_int32(-7)
        assert L.rt_scene_update_vertices(sc.handle, p, n - 1, _capi.UPDATE_AUTO, C.byref(out)) == _capi.RT_E_ARG
        assert L.rt_scene_update_vertices(sc.handle, p, n + 1, _capi.UPDATE_AUTO, C.byref(out)) == _capi.RT_E_ARG
        assert L.rt_scene_update_vertices(sc.handle, None, n, _capi.UPDATE_AUTO, C.byref(out)) == _capi.RT_E_ARG
        assert L.rt_scene_update_vertices(None, p, n, _capi.UPDATE_AUTO, C.byref(out)) == _capi.RT_E_ARG
        assert L.rt_scene_update_vertices(sc.handle, p, n, 2, C.byref(out)) == _capi.RT_E_ARG
        assert L.rt_scene_update_vertices(sc.handle, p, n, -1, C.byref(out)) == _capi.RT_E_ARG
        assert L.rt_scene_update_vertices_device(sc.handle, p, n, _capi.UPDATE_AUTO, C.byref(out)) == _capi.RT_E_NODEV
        assert L.rt_scene_update_vertices_device(None, p, n, _capi.UPDATE_AUTO, C.byref(out)) == _capi.RT_E_ARG
        assert out.value == -7
        e1 = sc.export()
        assert sc.bvh_digest() == d0
        assert np.array_equal(_bits(e1["vertices"]), _bits(e0["vertices"]))
        assert np.array_equal(_bits(e1["normals"]), _bits(e0["normals"]))
        # outcome may be NULL
        assert L.rt_scene_update_vertices(sc.handle, p, n, _capi.UPDATE_AUTO, None) == _capi.RT_OK
        assert np.array_equal(_bits(sc.export()["vertices"]), _bits(v))
        with pytest.raises(R.RtError):
            sc.update_vertices(v[:-1])


@pytest.mark.parametrize("name", ["one_triangle", "two_slivers"])
def test_tiny_scenes(name):
    v, t, moved = S.tiny_scenes()[name]
    mats = S.TINY_MATERIALS
    with R.Scene.create(v, t, np.zeros(len(t), np.uint32), mats, device=R.RT_HOST_ONLY) as sc, \
            R.Scene.create(moved, t, np.zeros(len(t), np.uint32), mats, device=R.RT_HOST_ONLY) as fresh:
        info = sc.bvh_info()
        if name == "one_triangle":
            assert info["leaf_triangles"] == 1 and info["nodes4"] == 1
        else:
            assert info["leaf_triangles"] == 0 and info["always"] == 2
        assert sc.update_vertices(moved) == "refit"
        sc.bvh_validate()
        assert sc.bvh_info() == info
        assert sc.bvh_digest() == fresh.bvh_digest()   # (one node: the refit is the fresh tree)
        assert np.array_equal(_bits(sc.export()["vertices"]), _bits(moved))
