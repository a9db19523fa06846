"""Dynamic geometry on the device (rt_scene_update_vertices / _device: k_refit_tris, k_refit_level4,
k_refit_level2): after an update every entry gives the bytes of a scene freshly created from the same
arrays, and of the oracle loading the same vertices from an OBJ.

Scene S and the deformations are tests/_refit_scenes.py's; frames are 96x64, pf 1, max_lvl 2, two lights,
every feature on. Equality is of bytes throughout.
"""
import os

import numpy as np
import pytest

import oracle as O
import raytracert_amd as R

import _refit_scenes as S

pytestmark = pytest.mark.gpu

W, H = S.W, S.H
P = R.RenderParams(width=W, height=H, pf=1, max_lvl=2, lights=S.LIGHTS)
OP = None


def _op():
    global OP
    if OP is None:
        OP = O.make_params(W, H, pf=1, max_lvl=2, lights=S.LIGHTS)
    return OP


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def arr(workdir):
    return S.base_arrays(workdir)


@pytest.fixture(scope="module")
def d003(arr, workdir, gpu_available):
    """D(0.03): the vertices, the oracle scene and frame, and a fresh device scene's frame (computed once)."""
    new = S.deform(arr["vertices"], 0.03)
    orc = S.oracle_scene(arr, new, workdir, "gpu_refit_d003")
    _, ou8, _ = orc.render(_op(), nthreads=16)
    with S.create(arr, new, device=0) as fresh:
        fu8, _, _ = fresh.render(P)
    assert np.array_equal(fu8, ou8)
    assert len(np.unique(ou8.reshape(-1, 3), axis=0)) > 50   # a frame with something in it
    return dict(vertices=new, oracle=orc, frame=ou8)


def _frames_all_modes(sc):
    out = {}
    sc.tune("bvh_width", 4)
    out["width4"] = sc.render(P)[0]
    sc.tune("bvh_width", 2)
    out["width2"] = sc.render(P)[0]
    sc.tune("bvh_width", 4)
    sc.set_accel("brute_force")
    out["brute_force"] = sc.render(P)[0]
    sc.set_accel("bvh")
    return out


def test_refit_frames_and_queries_equal_fresh_and_oracle(arr, d003):
    with S.create(arr, device=0) as sc:
        first = sc.render(P)[0]   # (the scene has rendered before: pipelines, orders and workspaces exist)
        assert sc.update_vertices(d003["vertices"]) == "refit"
        for mode, u8 in _frames_all_modes(sc).items():
            assert np.array_equal(u8, d003["frame"]), mode
        assert not np.array_equal(first, d003["frame"])
        # intersectMesh: rays from the camera over the frame and at the sliver, leaf and always records
        rng = np.random.default_rng(5)
        cs = R.default_corners(W, H)
        t = rng.uniform(0, 1, (200, 2)).astype(np.float32)
        o = np.tile(np.array(P.camera_pos, np.float32), (200, 1))
        d = (cs[1] * (1 - t[:, :1]) * (1 - t[:, 1:]) + cs[3] * (1 - t[:, :1]) * t[:, 1:] + cs[5] * t[:, :1] * (1 - t[:, 1:]) +
             cs[7] * t[:, :1] * t[:, 1:]).astype(np.float32)
        sliver = d003["vertices"][arr["n_grid_vertices"]:arr["n_grid_vertices"] + 3]
        d[:20] = (sliver[0] + (sliver[1] - sliver[0]) * t[:20, :1] + (sliver[2] - sliver[1]) * t[:20, :1] * t[:20, 1:]).astype(np.float32)
        idx, pts = sc.intersect_mesh(o, d)
        hits_sliver = 0
        for i in range(200):
            oi, oI = d003["oracle"].intersect_mesh(o[i], d[i])
            assert idx[i] == oi, i
            assert np.array_equal(_bits(pts[i]), _bits(oI)), i
            hits_sliver += oi == 1640
        assert hits_sliver > 0 and (idx >= 0).sum() > 50
        # one chain of trace() calls: normals, shadow rays
        k = int(np.argmax(idx[20:] >= 0)) + 20
        gb, grgb = sc.debug_trace(P, o[k], d[k])
        ob, _ = d003["oracle"].debug_trace(_op(), o[k], d[k])
        assert len(gb) == len(ob) and len(gb) >= 1
        for x, y in zip(gb, ob):
            for key in ("origin", "dest", "hit"):
                assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), key
            for key in ("triangle", "level", "shadowed", "lit"):
                assert x[key] == y[key], key
        prgb, _ = sc.perform_ray_tracing(P, o[k][None], d[k][None])
        with S.create(arr, d003["vertices"], device=0) as fresh:
            frgb, _ = fresh.perform_ray_tracing(P, o[k][None], d[k][None])
        assert np.array_equal(_bits(prgb), _bits(frgb)) and np.array_equal(_bits(prgb[0]), _bits(grgb))


def test_device_tree_equals_the_host_refit(arr, d003):
    with S.create(arr, device=0) as sc, S.create(arr) as host:
        d0 = sc.bvh_digest()
        assert sc.update_vertices(d003["vertices"]) == "refit"
        assert host.update_vertices(d003["vertices"]) == "refit"
        assert sc.bvh_digest() == host.bvh_digest() != d0   # read back from the device, nodes4 re-quantised
        sc.bvh_validate()
        assert sc.bvh_info() == host.bvh_info()
        e, f = sc.export(), host.export()
        assert np.array_equal(_bits(e["vertices"]), _bits(d003["vertices"]))
        assert np.array_equal(_bits(e["normals"]), _bits(f["normals"]))
        # and back: the first tree's bytes
        assert sc.update_vertices(arr["vertices"]) == "refit"
        assert sc.bvh_digest() == d0


def test_gross_deformation_still_refits(arr, gpu_available):
    new = S.gross(arr)
    with S.create(arr, device=0) as sc, S.create(arr, new, device=0) as fresh:
        assert sc.update_vertices(new) == "refit"
        want = fresh.render(P)[0]
        for mode, u8 in _frames_all_modes(sc).items():
            assert np.array_equal(u8, want), mode
        assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50
        sc.bvh_validate()


@pytest.mark.parametrize("case", ["collapse", "squeeze"])
def test_class_change_rebuilds_on_the_device(arr, case, workdir, gpu_available):
    new = getattr(S, case)(arr)
    orc = S.oracle_scene(arr, new, workdir, "gpu_refit_" + case)
    _, ou8, _ = orc.render(_op(), nthreads=16)
    with S.create(arr, device=0) as sc, S.create(arr, new) as host:
        sc.render(P)
        assert sc.update_vertices(new) == "rebuilt"
        for mode, u8 in _frames_all_modes(sc).items():
            assert np.array_equal(u8, ou8), mode
        assert sc.bvh_digest() == host.bvh_digest()
        # the rebuilt topology refits in turn
        back = S.deform(new, 0.01)
        assert sc.update_vertices(back) == "refit"
        with S.create(arr, back, device=0) as fresh:
            assert np.array_equal(sc.render(P)[0], fresh.render(P)[0])


def test_updates_are_ordered_with_frames_in_flight(arr, gpu_available):
    import torch
    dev = torch.device("cuda", 0)
    cs0 = R.default_corners(W, H)
    cs1 = (cs0 + np.array([0.05, 0.02, 0.0], np.float32)).astype(np.float32)
    views = [R.RenderParams(width=W, height=H, pf=1, max_lvl=2, lights=S.LIGHTS, corners=c) for c in (cs0, cs1)]
    verts = [S.deform(arr["vertices"], 0.01 * k) for k in range(1, 5)]
    want = []
    for v in verts:
        with S.create(arr, v, device=0) as fresh:
            want.append([fresh.render(q)[0] for q in views])
    assert not np.array_equal(want[0][0], want[3][0])
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    bufs = [[torch.full((H * W * 3,), 7, dtype=torch.uint8, device=dev) for _ in views] for _ in verts]
    torch.cuda.synchronize(dev)
    with S.create(arr, device=0) as sc:
        sc.tune("frames_in_flight", 2)
        cviews = [q.to_c() for q in views]
        for k, v in enumerate(verts):
            assert sc.update_vertices(v) == "refit"
            sc.render_frames_device(cviews, 16, 16, [b.data_ptr() for b in bufs[k]], H * W * 3, streams[k % 2].cuda_stream)
        torch.cuda.synchronize(dev)
        for k in range(len(verts)):
            for f in range(len(views)):
                assert np.array_equal(bufs[k][f].cpu().numpy().reshape(H, W, 3), want[k][f]), (k, f)


def test_device_pointer_entry(arr, d003):
    import torch
    with S.create(arr, device=0) as sc:
        sc.render(P)
        t = torch.from_numpy(d003["vertices"]).to("cuda:0")
        assert sc.update_vertices(t) == "refit"
        assert np.array_equal(sc.render(P)[0], d003["frame"])
        assert np.array_equal(_bits(sc.export()["vertices"]), _bits(d003["vertices"]))   # the lazy host refresh
        # a rebuild after a device-pointer update reads the vertices back
        new = S.collapse(arr)
        assert sc.update_vertices(torch.from_numpy(new).to("cuda:0")) == "rebuilt"
        with S.create(arr, new) as host:
            assert sc.bvh_digest() == host.bvh_digest()
        assert np.array_equal(_bits(sc.export()["vertices"]), _bits(new))


def test_scene_m1_follows_the_vertices(arr, gpu_available):
    """scene_m1 feeds the per-ray pad and the effective width (above 1e6 the binary tree is traversed)."""
    far = arr["vertices"].copy()
    far[arr["n_grid_vertices"] - 3, 0] = 50.0   # one back-plane vertex
    with S.create(arr, device=0) as sc, S.create(arr, far, device=0) as fresh:
        assert sc.update_vertices(far) == "refit"
        assert np.array_equal(sc.render(P)[0], fresh.render(P)[0])
    k = np.float32(2.0 ** 22)   # a power of two: every class stays (the arithmetic scales exactly)
    big = (arr["vertices"] * k).astype(np.float32)
    q = R.RenderParams(width=W, height=H, pf=1, max_lvl=2, lights=[tuple(float(x) * float(k) for x in l) for l in S.LIGHTS],
                       camera_pos=tuple(float(x) * float(k) for x in P.camera_pos), corners=R.default_corners(W, H) * k)
    with S.create(arr, device=0) as sc, S.create(arr, big, device=0) as fresh:
        sc.render(P)
        assert sc.update_vertices(big) == "refit"
        want = fresh.render(q)[0]
        assert np.array_equal(sc.render(q)[0], want)
        assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50
        # and back below 1e6: the four-wide tree again
        assert sc.update_vertices(arr["vertices"]) == "refit"
        with S.create(arr, device=0) as first:
            assert np.array_equal(sc.render(P)[0], first.render(P)[0])


@pytest.mark.parametrize("name", ["one_triangle", "two_slivers"])
def test_tiny_scenes_against_the_oracle(name, workdir, gpu_available):
    """The root is a leaf / the tree is empty. The slivers are thinner than a pixel of a 16x16 frame, so
    rays aimed at every triangle's centroid are compared as well."""
    from raytracert_amd import scenes
    v, t, moved = S.tiny_scenes()[name]
    scenes.write_sphere_grid(S.GRID, workdir, "refit_grid")   # (its MTL)

    def obj(vertices, stem):
        path = os.path.join(workdir, stem + ".obj")
        with open(path, "w") as f:
            f.write("mtllib refit_grid.mtl\nusemtl Sph0\n")
            for x, y, z in vertices:
                f.write("v %.9g %.9g %.9g\n" % (x, y, z))
            for a, b, c in t:
                f.write("f %d %d %d\n" % (a + 1, b + 1, c + 1))
        return path

    p = R.RenderParams(width=16, height=16, pf=1, max_lvl=2, lights=S.LIGHTS)
    op = O.make_params(16, 16, pf=1, max_lvl=2, lights=S.LIGHTS)
    orc = O.OracleScene(obj(moved, name + "_moved"))
    assert np.array_equal(_bits(orc.export()["vertices"]), _bits(moved))
    _, ou8, _ = orc.render(op, nthreads=4)
    o = np.tile(np.array(P.camera_pos, np.float32), (len(t), 1))
    d = np.array([moved[tri].mean(axis=0) for tri in t], np.float32)
    want = [orc.intersect_mesh(o[i], d[i]) for i in range(len(t))]
    assert [w[0] for w in want] == list(range(len(t)))
    with R.Scene.load(obj(v, name), device=0) as sc:
        before = sc.render(p)[0]
        assert sc.update_vertices(moved) == "refit"
        for mode in ("bvh", "brute_force"):
            sc.set_accel(mode)
            assert np.array_equal(sc.render(p)[0], ou8), mode
            idx, pts = sc.intersect_mesh(o, d)
            for i, (wi, wI) in enumerate(want):
                assert idx[i] == wi and np.array_equal(_bits(pts[i]), _bits(wI)), (mode, i)
        sc.bvh_validate()
        if name == "one_triangle":
            assert ou8.max() > 0 and not np.array_equal(before, ou8)
