"""Topology changes on the host (rt_scene_set_mesh on host-only scenes): after a replacement the scene is,
bit for bit, the scene rt_scene_create_ex makes from the same arrays, the scene's materials and the scene's
builder. One scene per builder is walked through a chain of meshes that grows and shrinks (to nothing and
back); the device path has the same contract in tests/test_gpu_set_mesh.py.
"""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

import _lbvh_scenes as L

BUILDERS = ("sah", "lbvh", "cluster")
OUTCOME = {"sah": "rebuilt", "lbvh": "rebuilt_lbvh", "cluster": "rebuilt_cluster"}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "models")


def chain(workdir):
    """(name, vertices, triangles): counts go up, down, to zero, up again, and end with shared vertices."""
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    return [("soup5",) + L.soup_exact(5), ("mixed2049",) + L.soup(2049, 7, always=0.1, never=0.1), ("soup3",) + L.soup_exact(3),
            ("empty",) + empty, ("soup65",) + L.soup_exact(65), ("grid",) + L.indexed_grid(workdir)]


def tri_mats(nt):
    """Both of _lbvh_scenes.MATERIALS' entries in use where there are two."""
    return (np.arange(nt, dtype=np.uint32) % np.uint32(len(L.MATERIALS))).astype(np.uint32)


def same_scene(sc, fresh, what):
    assert sc.counts() == fresh.counts(), what
    assert sc.bvh_digest() == fresh.bvh_digest(), what
    assert sc.bvh_info() == fresh.bvh_info(), what
    for a, b in zip(sc.bvh_order(), fresh.bvh_order()):
        assert np.array_equal(a, b), what
    e, f = sc.export(), fresh.export()
    for k in ("vertices", "triangles", "tri_mat", "normals"):
        assert e[k].shape == f[k].shape and e[k].tobytes() == f[k].tobytes(), (what, k)
    assert e["materials"] == f["materials"], what
    sc.bvh_validate()


@pytest.mark.parametrize("builder", BUILDERS)
def test_chain_of_meshes_equals_fresh_scenes(builder, workdir):
    meshes = chain(workdir)
    assert len(meshes[-1][2]) > len(meshes[-1][1])   # nt > nv
    v0, t0 = L.soup_exact(9)
    with R.Scene.create(v0, t0, tri_mats(len(t0)), L.MATERIALS, device=R.RT_HOST_ONLY, builder=builder) as sc:
        for name, v, t in meshes:
            m = tri_mats(len(t))
            out = sc.set_mesh(v, t, m)
            with R.Scene.create(v, t, m, L.MATERIALS, device=R.RT_HOST_ONLY, builder=builder) as fresh:
                same_scene(sc, fresh, name)
                assert sc.builder == fresh.builder and sc.build_info() == fresh.build_info(), name
                assert out == OUTCOME[fresh.builder[1]], (name, out)   # *outcome reports the builder, as an update's
                if len(t) > 2:
                    assert out == OUTCOME[builder], (name, out)
                for i in (0, len(t) // 2, len(t) - 1):
                    if len(t):
                        assert sc.get_material(i) == fresh.get_material(i), name
                # a later update refits the tree the replacement built
                if len(v):
                    assert sc.update_vertices(L.move(v)) == "refit", name
                    assert fresh.update_vertices(L.move(v)) == "refit", name
                    same_scene(sc, fresh, name + " moved")


def _export_bytes(sc):
    e = sc.export()
    return sc.counts(), tuple(e[k].tobytes() for k in ("vertices", "triangles", "tri_mat", "normals")), sc.bvh_digest()


@pytest.mark.parametrize("builder", BUILDERS)
def test_rejected_meshes_leave_the_scene_alone(builder):
    v0, t0 = L.soup_exact(65)
    v, t = L.soup_exact(5)
    nv, nm = len(v), len(L.MATERIALS)
    cases = []
    bad = t.copy(); bad[3, 1] = nv
    cases.append((bad, tri_mats(5), "triangle references a missing vertex"))
    bad = t.copy(); bad[4, 2] = 0xFFFFFFFF
    cases.append((bad, tri_mats(5), "triangle references a missing vertex"))
    badm = tri_mats(5); badm[2] = nm
    cases.append((t, badm, "triangle references a missing material"))
    with R.Scene.create(v0, t0, tri_mats(65), L.MATERIALS, device=R.RT_HOST_ONLY, builder=builder) as sc:
        before = _export_bytes(sc)
        for tri, mat, text in cases:
            with pytest.raises(_capi.RtError) as ei:
                sc.set_mesh(v, tri, mat)
            assert ei.value.code == _capi.RT_E_PARSE and text in str(ei.value)
            # creation rejects the same arrays with the same text
            with pytest.raises(_capi.RtError) as ec:
                R.Scene.create(v, tri, mat, L.MATERIALS, device=R.RT_HOST_ONLY, builder=builder)
            assert ec.value.code == _capi.RT_E_PARSE and text in str(ec.value)
            assert _export_bytes(sc) == before
        sc.bvh_validate()


def test_argument_errors_and_the_device_entry_on_a_host_scene():
    v, t = L.soup_exact(5)
    m = tri_mats(5)
    lib = _capi.lib()
    out = C.c_int32(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    with L.create(v, t) as sc:
        before = _export_bytes(sc)
        h = sc.handle
        assert lib.rt_scene_set_mesh_device(h, vp(v), len(v), vp(t), vp(m), 5, None, C.byref(out)) == _capi.RT_E_NODEV
        assert lib.rt_scene_set_mesh_device(None, vp(v), len(v), vp(t), vp(m), 5, None, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh(None, vp(v), len(v), vp(t), vp(m), 5, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh(h, vp(v), -1, vp(t), vp(m), 5, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh(h, vp(v), len(v), vp(t), vp(m), -1, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh(h, None, len(v), vp(t), vp(m), 5, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh(h, vp(v), len(v), None, vp(m), 5, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh(h, vp(v), len(v), vp(t), None, 5, C.byref(out)) == _capi.RT_E_ARG
        assert out.value == -1 and _export_bytes(sc) == before
        # NULL arrays with zero counts, and no outcome pointer
        assert lib.rt_scene_set_mesh(h, None, 0, None, None, 0, None) == _capi.RT_OK
        assert sc.counts()[:2] == (0, 0)
        assert lib.rt_scene_set_mesh(h, vp(v), len(v), vp(t), vp(m), 5, C.byref(out)) == _capi.RT_OK
        assert out.value == _capi.UPDATED_REBUILT_LBVH and _capi.MESH_REPLACED == _capi.RT_OK
        with pytest.raises(ValueError):
            sc.set_mesh(v, t, m[:4])
        with pytest.raises(ValueError):
            sc.set_mesh(v, t, m, counts=np.array([3, 1], np.int32))


def test_texture_coordinates_are_dropped(tmp_path):
    p = tmp_path / "cube.obj"
    p.write_text(gzip.open(os.path.join(GOLDEN, "cube.obj.gz"), "rt").read())
    v, t = L.soup_exact(5)
    with R.Scene.load(str(p), device=R.RT_HOST_ONLY, texcoords=True) as sc:
        tc, tt = sc.texcoords()
        assert len(tc) == 4 and tt.any()
        nm = sc.counts()[2]
        sc.set_mesh(v, t, np.zeros(5, np.uint32))
        tc, tt = sc.texcoords()
        assert tc.shape == (0, 3) and tt.shape == (5, 3) and not tt.any()
        assert sc.counts() == (15, 5, nm)   # the material table stays
    with R.Scene.load(str(p), device=R.RT_HOST_ONLY) as sc:     # a scene without them still has none to report
        sc.set_mesh(v, t, np.zeros(5, np.uint32))
        with pytest.raises(_capi.RtError):
            sc.texcoords()
