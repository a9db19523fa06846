"""Topology changes on the device (rt_scene_set_mesh / rt_scene_set_mesh_device: k_mesh_validate,
k_mesh_transparent, then k_refit_tris and the device builders): after a replacement every entry gives the
bytes of a scene freshly created from the same arrays, the scene's materials and the scene's builder.

Meshes are tests/_lbvh_scenes.py's, materials and rays tests/_query_scenes.py's. Equality is of bytes
throughout. Host statements and fresh scenes' answers are computed once per (builder, mesh) and shared.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _lbvh_scenes as L
import _query_scenes as QS
import _refit_scenes as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUTCOME = {"sah": "rebuilt", "lbvh": "rebuilt_lbvh", "cluster": "rebuilt_cluster"}
EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
MESHES = {
    **{"np%d" % n: functools.partial(L.soup_exact, n) for n in (2, 3, 5, 64, 65, 256, 257, 2047, 2049, 8193)},
    "empty": lambda: EMPTY,
    "mixed2049": functools.partial(L.soup, 2049, 7, 0.1, 0.1),
    "lattice3000": functools.partial(L.lattice, 3000),
}
# One scene walks this: up and down across RT_BVH_MAX_LEAF (2, 3, 5), the wave (64, 65), the block (256, 257),
# kLbvhSortItems (2047, 2049) and kScanBlock (8193); 5 -> 8193 grows every buffer, 8193 -> 3 -> 2049 reuses them.
WALK = ["np5", "np8193", "np3", "np2049", "np2", "np3", "np5", "np2", "np65", "np64", "np65", "np257", "np256", "np257",
        "np2049", "np2047", "mixed2049", "empty", "lattice3000", "np2047", "np8193", "empty", "np5"]
QUERIED = ("np2049", "lattice3000", "np8193")
ORIGIN = np.array([0.3, -0.2, 3.5], np.float32)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, t = MESHES[name]()
    v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.uint32)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def _dev(v, t, m):
    """The three arrays as CUDA tensors (the indices as int32 words)."""
    return (torch.from_numpy(np.array(v, np.float32)).to(DEV), torch.from_numpy(np.array(t, np.uint32).view(np.int32)).to(DEV),
            torch.from_numpy(np.array(m, np.uint32).view(np.int32)).to(DEV))


@functools.lru_cache(maxsize=None)
def _host(builder, name):
    """The host statement: a host-only fresh scene of the builder."""
    v, t = _mesh(name)
    with L.create(v, t, builder=builder) as h:
        return dict(digest=h.bvh_digest(), info=h.bvh_info(), built=h.builder)


def _rays(v, t, seed=21, n=4096):
    """n fixed-seed rays from ORIGIN: three quarters at centroids of random triangles, the rest at random
    points of the plane z = 0 (some leave the scene)."""
    rng = np.random.default_rng(seed)
    k = 3 * n // 4
    aimed = v[t[rng.integers(0, len(t), k)].astype(np.int64)].astype(np.float64).mean(axis=1)
    loose = np.concatenate([rng.uniform(-2, 2, (n - k, 2)), np.zeros((n - k, 1))], axis=1)
    d = np.concatenate([aimed, loose]).astype(np.float32)
    return np.tile(ORIGIN, (n, 1)).astype(np.float32), d


def _all_traversals(sc, o, d):
    out = []
    for width in (4, 2):
        sc.tune("bvh_width", width)
        out.append(sc.intersect_mesh(o, d))
    sc.tune("bvh_width", 4)
    sc.set_accel("brute_force")
    out.append(sc.intersect_mesh(o, d))
    sc.set_accel("bvh")
    return [(i.tobytes(), _bits(p).tobytes()) for i, p in out]


@functools.lru_cache(maxsize=None)
def _fresh_answers(builder, name):
    v, t = _mesh(name)
    o, d = _rays(v, t)
    with L.create(v, t, device=0, builder=builder) as fresh:
        idx, pts = fresh.intersect_mesh(o, d)
        assert (idx >= 0).sum() >= 1024 and (idx < 0).sum() >= 64, "the comparison must not pass on misses alone"
        return idx.tobytes(), _bits(pts).tobytes()


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["lbvh", "cluster"])
def test_one_scene_through_every_size_boundary(builder, gpu_available):
    v0, t0 = L.soup_exact(9)
    with L.create(v0, t0, device=0, builder=builder) as sc:
        for step, name in enumerate(WALK):
            v, t = _mesh(name)
            want = _host(builder, name)
            assert sc.set_mesh(*_dev(v, t, np.zeros(len(t), np.uint32))) == OUTCOME[want["built"][1]], (step, name)
            if len(t) > 2:
                assert want["built"] == (builder, builder), (step, name)
            assert sc.counts() == (len(v), len(t), 1), (step, name)
            assert sc.builder == want["built"], (step, name)
            assert sc.bvh_digest() == want["digest"], (step, name)
            assert sc.bvh_info() == want["info"], (step, name)
            sc.bvh_validate()
            e = sc.export()
            assert e["vertices"].tobytes() == v.tobytes() and e["triangles"].tobytes() == t.tobytes(), (step, name)
            assert not e["tri_mat"].any() and e["tri_mat"].shape == (len(t),)
            if name in QUERIED:
                o, d = _rays(v, t)
                for got in _all_traversals(sc, o, d):
                    assert got == _fresh_answers(builder, name), (step, name)
        # a later update refits the trees the last replacement built
        v, t = _mesh(WALK[-1])
        assert sc.update_vertices(torch.from_numpy(L.move(v)).to(DEV)) == "refit"
        with L.create(v, t, builder=builder) as h:
            assert h.update_vertices(L.move(v)) == "refit"
            assert sc.bvh_digest() == h.bvh_digest()


# 2 -------------------------------------------------------------------------------------------------
def test_sah_builder_rebuilds_on_the_host(gpu_available):
    v0, t0 = L.soup_exact(9)
    with L.create(v0, t0, device=0, builder="sah") as sc:
        for k, name in enumerate(["np5", "np2049", "np65"]):
            v, t = _mesh(name)
            m = np.zeros(len(t), np.uint32)
            out = sc.set_mesh(v, t, m) if k == 1 else sc.set_mesh(*_dev(v, t, m))   # (host arrays once)
            assert out == "rebuilt" and sc.builder == ("sah", "sah"), name
            want = _host("sah", name)
            assert sc.counts() == (len(v), len(t), 1)
            assert sc.bvh_digest() == want["digest"] and sc.bvh_info() == want["info"], name
            sc.bvh_validate()
            e = sc.export()
            assert e["vertices"].tobytes() == v.tobytes() and e["triangles"].tobytes() == t.tobytes(), name
        o, d = _rays(*_mesh("np65"), n=512)
        with L.create(*_mesh("np65"), device=0, builder="sah") as fresh:
            fi, fp = fresh.intersect_mesh(o, d)
        assert (fi >= 0).sum() >= 128
        for got in _all_traversals(sc, o, d):
            assert got == (fi.tobytes(), _bits(fp).tobytes())


# 3, 4: scenes with Q's materials (Sph2, index 3, is transparent) -----------------------------------
@pytest.fixture(scope="module")
def qmats(workdir, gpu_available):
    path = scenes.write_sphere_grid(QS.SPEC_Q, workdir, "set_mesh_q")
    with R.Scene.load(path, device=R.RT_HOST_ONLY) as sc:
        e = sc.export()
    mats = e["materials"]
    transparent = [bool(m["flags"] & QS.HAS_TR) and m["Tr"] < 1 for m in mats]
    assert len(mats) == len(S.MTL_NAMES) and transparent == [False, False, False, True, False]
    return dict(materials=mats, mtl=path[:-4] + ".mtl", q=e)


FW, FH = 64, 48
FP = R.RenderParams(width=FW, height=FH, pf=1, max_lvl=3, lights=S.LIGHTS)


def test_frames_follow_the_mesh(qmats, workdir):
    va, ta = L.indexed_grid(workdir)
    ma = (1 + np.arange(len(ta), dtype=np.uint32) % 2).astype(np.uint32)            # opaque Sph0 / Sph1
    vb, tb = _mesh("mixed2049")
    mb = (1 + np.arange(len(tb), dtype=np.uint32) % 4).astype(np.uint32)            # every fourth one transparent
    arr_b = dict(triangles=tb, tri_mat=mb, mtl=qmats["mtl"])
    orc = S.oracle_scene(arr_b, vb, workdir, "set_mesh_b")
    _, ou8, _ = orc.render(O.make_params(FW, FH, pf=1, max_lvl=3, lights=S.LIGHTS), nthreads=16)
    with R.Scene.create(vb, tb, mb, qmats["materials"], device=0, builder="lbvh") as fresh:
        fb = fresh.render(FP)[0]
    assert np.array_equal(fb, ou8) and len(np.unique(ou8.reshape(-1, 3), axis=0)) > 10
    for builder in ("lbvh", "sah"):
        with R.Scene.create(va, ta, ma, qmats["materials"], device=0, builder=builder) as sc:
            first = sc.render(FP)[0]
            for _ in range(3):                                   # batch orders and launch trials of mesh A
                assert np.array_equal(sc.render(FP)[0], first)
            assert len(np.unique(first.reshape(-1, 3), axis=0)) > 50
            assert sc.set_mesh(vb, tb, mb) == OUTCOME[builder]   # host arrays
            for _ in range(2):
                assert np.array_equal(sc.render(FP)[0], ou8), builder
            for i in (0, 3, 2048):
                assert sc.get_material(i) == qmats["materials"][mb[i]]
            assert sc.set_mesh(*_dev(va, ta, ma)) == OUTCOME[builder]   # and back, from device arrays
            for _ in range(2):
                assert np.array_equal(sc.render(FP)[0], first), builder
            assert sc.get_material(1) == qmats["materials"][ma[1]]


def test_occlusion_shortcut_follows_the_mesh(qmats):
    q = qmats["q"]
    v, t, mb = q["vertices"], q["triangles"], q["tri_mat"]
    ma = np.where(mb == 3, np.uint32(2), mb).astype(np.uint32)        # A: Sph2's triangles opaque
    assert (mb == 3).sum() > 100
    o, d = QS.r200()
    do, dd = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    want = {}
    for key, m in (("a", ma), ("b", mb)):
        with R.Scene.create(v, t, m, qmats["materials"], device=0, builder="lbvh") as fresh:
            want[key] = fresh.occluded_device(do, dd).cpu().numpy()
    flips = want["a"] != want["b"]
    assert flips.sum() >= 10 and (want["a"][flips] == 1).all()         # transparent closest hits stop blocking
    with R.Scene.create(v, t, ma, qmats["materials"], device=0, builder="lbvh") as sc:
        assert np.array_equal(sc.occluded_device(do, dd).cpu().numpy(), want["a"])
        sc.set_mesh(*_dev(v, t, mb))                                   # A -> B: the any-hit walk must stop
        assert np.array_equal(sc.occluded_device(do, dd).cpu().numpy(), want["b"])
        sc.set_mesh(*_dev(v, t, ma))                                   # B -> A
        assert np.array_equal(sc.occluded_device(do, dd).cpu().numpy(), want["a"])
        sc.set_mesh(v, t, mb)                                          # host arrays: the host's table
        assert np.array_equal(sc.occluded_device(do, dd).cpu().numpy(), want["b"])


# 5 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["lbvh", "cluster"])
def test_device_counts_decide_the_live_mesh(builder, gpu_available):
    v, t = _mesh("np2049")
    live_t, live_v = 257, 3 * 257
    dv, dt, dm = _dev(v, t, np.zeros(len(t), np.uint32))
    dv[live_v:] = float("nan")
    dt[live_t:] = -1          # 0xFFFFFFFF: must never be looked at
    dm[live_t:] = -1
    counts = torch.tensor([live_v, live_t], dtype=torch.int32, device=DEV)
    with L.create(*_mesh("np5"), device=0, builder=builder) as sc, \
            L.create(v[:live_v], t[:live_t], builder=builder) as h:
        assert sc.set_mesh(dv, dt, dm, counts=counts) == OUTCOME[builder]
        assert sc.counts() == (live_v, live_t, 1)
        assert sc.bvh_digest() == h.bvh_digest() and sc.bvh_info() == h.bvh_info()
        sc.bvh_validate()
        e = sc.export()
        assert e["vertices"].tobytes() == v[:live_v].tobytes() and e["triangles"].tobytes() == t[:live_t].tobytes()
        o, d = _rays(v[:live_v], t[:live_t], n=512)
        with L.create(v[:live_v], t[:live_t], device=0, builder=builder) as fresh:
            fi, fp = fresh.intersect_mesh(o, d)
        assert (fi >= 0).sum() >= 128
        gi, gp = sc.intersect_mesh(o, d)
        assert np.array_equal(gi, fi) and np.array_equal(_bits(gp), _bits(fp))
        # counts beyond the capacities are clamped to them, negative ones to zero
        dv2, dt2, dm2 = _dev(v[:live_v], t[:live_t], np.zeros(live_t, np.uint32))
        assert sc.set_mesh(dv2, dt2, dm2, counts=torch.tensor([1 << 30, 1 << 30], dtype=torch.int32, device=DEV)).startswith("rebuilt")
        assert sc.counts() == (live_v, live_t, 1) and sc.bvh_digest() == h.bvh_digest()
        sc.set_mesh(dv2, dt2, dm2, counts=torch.tensor([live_v, -4], dtype=torch.int32, device=DEV))
        assert sc.counts() == (live_v, 0, 1)


# 6 -------------------------------------------------------------------------------------------------
def test_stream_order_with_queries_in_flight(gpu_available):
    va, ta = _mesh("np2049")
    vb, tb = _mesh("lattice3000")
    reps = 25
    st = torch.cuda.Stream(device=DEV)
    oa, da = _rays(va, ta)
    o = np.tile(oa, (reps, 1))
    d = np.tile(da, (reps, 1))
    assert len(o) == 102400
    want = {}
    for key, (v, t) in (("a", (va, ta)), ("b", (vb, tb))):
        with L.create(v, t, device=0) as fresh:
            want[key] = fresh.intersect_mesh(oa, da)
    assert not np.array_equal(want["a"][0], want["b"][0])
    mesh_b = _dev(vb, tb, np.zeros(len(tb), np.uint32))
    with L.create(va, ta, device=0) as sc:
        do, dd = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            idx1, pts1 = sc.intersect_mesh_device(do, dd)
        assert sc.set_mesh(*mesh_b) == "rebuilt_lbvh"       # at once: the queries above are still in flight
        with torch.cuda.stream(st):
            idx2, pts2 = sc.intersect_mesh_device(do, dd)
        st.synchronize()
        for (idx, pts), key in (((idx1, pts1), "a"), ((idx2, pts2), "b")):
            wi, wp = want[key]
            assert np.array_equal(idx.cpu().numpy().reshape(reps, -1), np.tile(wi, (reps, 1))), key
            assert np.array_equal(_bits(pts).reshape(reps, -1, 3), np.tile(_bits(wp), (reps, 1, 1))), key


# 7 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["lbvh", "sah"])
def test_rejected_device_meshes_leave_the_scene_alone(builder, gpu_available):
    """Error handling only: the vertex tensor is a slice of a larger allocation, so even an implementation
    that dereferenced the bad index would stay inside allocated memory; a correct one never loads a vertex
    before the verdict."""
    v0, t0 = _mesh("np257")
    v, t = _mesh("np65")
    nv, nt = len(v), len(t)
    big = torch.zeros((nv + 64, 3), dtype=torch.float32, device=DEV)
    big[:nv] = torch.from_numpy(np.array(v)).to(DEV)
    dv = big[:nv]
    _, dt, dm = _dev(v, t, np.zeros(nt, np.uint32))
    bad_t = dt.clone(); bad_t[40, 1] = nv
    bad_m = dm.clone(); bad_m[33] = 1                      # == n_materials
    o, d = _rays(v0, t0)
    with L.create(v0, t0, device=0, builder=builder) as sc:
        digest, answers, counts = sc.bvh_digest(), sc.intersect_mesh(o, d), sc.counts()
        assert (answers[0] >= 0).sum() >= 1024
        for tri, mat, text in ((bad_t, dm, "triangle references a missing vertex"), (dt, bad_m, "triangle references a missing material")):
            with pytest.raises(_capi.RtError) as ei:
                sc.set_mesh(dv, tri, mat)
            assert ei.value.code == _capi.RT_E_PARSE and text in str(ei.value)
            assert sc.counts() == counts and sc.bvh_digest() == digest
            gi, gp = sc.intersect_mesh(o, d)
            assert np.array_equal(gi, answers[0]) and np.array_equal(_bits(gp), _bits(answers[1]))
        # the argument checks of the device entry
        lib, out = _capi.lib(), C.c_int32(-1)
        vp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
        h = sc.handle
        assert lib.rt_scene_set_mesh_device(h, vp(dv, 2), nv - 1, vp(dt), vp(dm), nt, None, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh_device(h, vp(dv), nv, vp(dt), vp(dm, 1), nt - 1, None, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh_device(h, vp(dv), nv, None, vp(dm), nt, None, C.byref(out)) == _capi.RT_E_ARG
        assert lib.rt_scene_set_mesh_device(h, vp(dv), -1, vp(dt), vp(dm), nt, None, C.byref(out)) == _capi.RT_E_ARG
        assert out.value == -1 and sc.bvh_digest() == digest
        with pytest.raises(ValueError):
            sc.set_mesh(dv, dt.cpu(), dm)
        with pytest.raises(ValueError):
            sc.set_mesh(dv, dt, dm, counts=torch.zeros(2, dtype=torch.int32))
        # and the same arrays, unspoilt, are taken
        assert sc.set_mesh(dv, dt, dm) == OUTCOME[builder] and sc.counts() == (nv, nt, 1)
