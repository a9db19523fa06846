"""The agglomerative GPU BVH build (RT_BUILD_CLUSTER on a device scene: the k_cluster_* kernels): the
device-built trees equal the host statement's bit for bit (rt_scene_bvh_digest), and every entry gives the
bytes of a SAH scene and of the oracle, as any valid tree must.

Scene S and the deformations are tests/_refit_scenes.py's; frames are 96x64, pf 1, max_lvl 2, two lights.
Equality is of bytes throughout.
"""
import numpy as np
import pytest

import oracle as O
import raytracert_amd as R

import _refit_scenes as S

pytestmark = pytest.mark.gpu

W, H = S.W, S.H
P = R.RenderParams(width=W, height=H, pf=1, max_lvl=2, lights=S.LIGHTS)


def _op():
    return O.make_params(W, H, pf=1, max_lvl=2, lights=S.LIGHTS)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _create(arr, vertices=None, device=0, builder="cluster"):
    return R.Scene.create(arr["vertices"] if vertices is None else vertices, arr["triangles"], arr["tri_mat"],
                          arr["materials"], device=device, builder=builder)


def _host(arr, vertices=None, builder="cluster"):
    return _create(arr, vertices, R.RT_HOST_ONLY, builder)


def copies70():
    v = np.tile(np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.1, 0.7, -0.2]], np.float32), (70, 1))
    return v, np.arange(210, dtype=np.uint32).reshape(70, 3)


@pytest.fixture(scope="module")
def arr(workdir):
    return S.base_arrays(workdir)


@pytest.fixture(scope="module")
def d001(arr):
    return S.deform(arr["vertices"], 0.01)


@pytest.fixture(scope="module")
def d003(arr, workdir, gpu_available):
    """D(0.03): the vertices, the oracle scene and frame, a fresh SAH device scene's frame, and the host
    statement's digest of the clustered tree of these vertices (computed once)."""
    new = S.deform(arr["vertices"], 0.03)
    orc = S.oracle_scene(arr, new, workdir, "gpu_cluster_d003")
    _, ou8, _ = orc.render(_op(), nthreads=16)
    with S.create(arr, new, device=0) as fresh:
        fu8, _, _ = fresh.render(P)
        assert fresh.builder == ("sah", "sah")
    assert np.array_equal(fu8, ou8)
    with _host(arr, new) as h:
        digest, info, build = h.bvh_digest(), h.bvh_info(), h.build_info()
        assert h.builder == ("cluster", "cluster")
    return dict(vertices=new, oracle=orc, frame=ou8, digest=digest, info=info, build=build)


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


def test_device_build_equals_the_host_statement(arr, gpu_available):
    with _create(arr) as sc, _host(arr) as host, S.create(arr) as sah:
        assert sc.builder == ("cluster", "cluster")
        assert sc.bvh_digest() == host.bvh_digest() != sah.bvh_digest()
        assert sc.bvh_info() == host.bvh_info()
        assert sc.build_info() == host.build_info() and sc.build_info()["iterations"] > 0
        sc.bvh_validate()   # the tree the kernels traverse, read back
        with _create(arr, builder="lbvh") as lb:   # the Morton builder's order, another topology
            assert np.array_equal(sc.bvh_order()[0], lb.bvh_order()[0]) and sc.bvh_digest() != lb.bvh_digest()


@pytest.mark.parametrize("name", ["one_triangle", "two_slivers", "copies70"])
def test_small_trees_equal_the_host_statement(name, gpu_available):
    v, t = copies70() if name == "copies70" else S.tiny_scenes()[name][:2]
    m = np.zeros(len(t), np.uint32)
    p = R.RenderParams(width=16, height=16, pf=1, max_lvl=2, lights=S.LIGHTS)
    with R.Scene.create(v, t, m, S.TINY_MATERIALS, device=0, builder="cluster") as sc, \
            R.Scene.create(v, t, m, S.TINY_MATERIALS, device=R.RT_HOST_ONLY, builder="cluster") as host, \
            R.Scene.create(v, t, m, S.TINY_MATERIALS, device=0) as sah:
        assert sc.builder == ("cluster", "cluster")
        frame = sc.render(p)[0]
        assert np.array_equal(frame, sah.render(p)[0])
        assert sc.bvh_digest() == host.bvh_digest()
        assert sc.bvh_info() == host.bvh_info()
        sc.bvh_validate()
        # and a refit of the device-made tables
        moved = (v * np.float32(1.25)).astype(np.float32)
        assert sc.update_vertices(moved) == "refit" and host.update_vertices(moved) == "refit"
        assert sc.bvh_digest() == host.bvh_digest()


def test_rebuild_from_host_array_and_device_tensor(arr, d003):
    import torch
    with _create(arr) as sc:
        sc.render(P)
        assert sc.update_vertices(d003["vertices"], mode="rebuild") == "rebuilt_cluster"
        assert sc.bvh_digest() == d003["digest"]
        sc.bvh_validate()
        assert np.array_equal(_bits(sc.export()["vertices"]), _bits(d003["vertices"]))
    with S.create(arr, device=0) as sc:   # a SAH scene switched over; vertices from device memory
        sc.render(P)
        sc.set_builder("cluster")
        assert sc.builder == ("cluster", "sah")
        t = torch.from_numpy(d003["vertices"]).to("cuda:0")
        assert sc.update_vertices(t, mode="rebuild") == "rebuilt_cluster"
        assert sc.builder == ("cluster", "cluster")
        assert np.array_equal(sc.render(P)[0], d003["frame"])
        assert sc.bvh_digest() == d003["digest"]
        assert sc.bvh_info() == d003["info"] and sc.build_info() == d003["build"]
        sc.bvh_validate()
        assert np.array_equal(_bits(sc.export()["vertices"]), _bits(d003["vertices"]))


def test_frames_queries_and_trace_equal_sah_and_oracle(arr, d003):
    with _create(arr, d003["vertices"]) as sc, S.create(arr, d003["vertices"], device=0) as sah:
        for mode, u8 in _frames_all_modes(sc).items():
            assert np.array_equal(u8, d003["frame"]), mode
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
        k = int(np.argmax(idx[20:] >= 0)) + 20
        gb, grgb = sc.debug_trace(P, o[k], d[k])
        sb, srgb = sah.debug_trace(P, o[k], d[k])
        assert len(gb) == len(sb) and len(gb) >= 1
        for x, y in zip(gb, sb):
            for key in ("origin", "dest", "hit"):
                assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), key
            for key in ("triangle", "level", "shadowed", "lit"):
                assert x[key] == y[key], key
        assert np.array_equal(_bits(grgb), _bits(srgb))


def test_class_change_rebuilds_on_the_device(arr, gpu_available):
    new = S.collapse(arr)
    with _create(arr) as sc, S.create(arr, new, device=0) as fresh, _host(arr, new) as host:
        first = sc.render(P)[0]
        assert sc.update_vertices(new) == "rebuilt_cluster"
        assert np.array_equal(sc.render(P)[0], fresh.render(P)[0])
        assert sc.bvh_digest() == host.bvh_digest()
        assert sc.update_vertices(arr["vertices"]) == "rebuilt_cluster"   # the class changes back
        assert np.array_equal(sc.render(P)[0], first)


def test_refit_after_a_device_build(arr, d001, d003):
    with _create(arr) as sc, _host(arr) as host:
        assert sc.update_vertices(d001, mode="rebuild") == "rebuilt_cluster"
        assert sc.update_vertices(d003["vertices"]) == "refit"      # the device-made tri_slot and level tables
        assert host.update_vertices(d001, mode="rebuild") == "rebuilt_cluster"
        assert host.update_vertices(d003["vertices"]) == "refit"
        for mode, u8 in _frames_all_modes(sc).items():
            assert np.array_equal(u8, d003["frame"]), mode
        assert sc.bvh_digest() == host.bvh_digest()
        sc.bvh_validate()


def test_rebuild_between_frames_in_flight(arr, d003):
    import torch
    dev = torch.device("cuda", 0)
    bufs = [torch.full((H * W * 3,), 7, dtype=torch.uint8, device=dev) for _ in range(4)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize(dev)
    with S.create(arr, device=0) as sc, S.create(arr, device=0) as first:
        sc.tune("frames_in_flight", 2)
        sc.set_builder("cluster")
        c = P.to_c()
        for k in (0, 1):   # (both pipelines have their workspaces)
            sc.render_frame_device(c, 16, 16, bufs[k].data_ptr(), H * W * 3, streams[k].cuda_stream)
        ws = sc.workspace_bytes()
        assert sc.update_vertices(d003["vertices"], mode="rebuild") == "rebuilt_cluster"   # (the frames above still in flight)
        for k in (2, 3):
            sc.render_frame_device(c, 16, 16, bufs[k].data_ptr(), H * W * 3, streams[k & 1].cuda_stream)
        torch.cuda.synchronize(dev)
        want0 = first.render(P)[0]
        for k in range(4):
            assert np.array_equal(bufs[k].cpu().numpy().reshape(H, W, 3), want0 if k < 2 else d003["frame"]), k
        assert sc.workspace_bytes() == ws


def test_repeated_rebuilds_leave_no_stale_scratch(arr, d001, d003):
    with _host(arr, d001) as h:
        want = {0: h.bvh_digest(), 1: d003["digest"]}
    assert want[0] != want[1]
    with _create(arr) as sc:
        for k in range(5):
            v = d003["vertices"] if k & 1 else d001
            assert sc.update_vertices(v, mode="rebuild") == "rebuilt_cluster"
            assert sc.bvh_digest() == want[k & 1], k


def test_fallback_on_the_device(arr, d003, monkeypatch):
    with _create(arr) as sc, S.create(arr, d003["vertices"]) as sah:
        assert sc.builder == ("cluster", "cluster")
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", "12")   # too deep for the clustered and the Morton tree: the SAH builder
        assert sc.update_vertices(d003["vertices"], mode="rebuild") == "rebuilt"
        assert sc.builder == ("cluster", "sah") and sc.build_info()["fallback"] == "depth"
        assert sc.build_info()["iterations"] == 0
        assert np.array_equal(sc.render(P)[0], d003["frame"])
        assert sc.bvh_digest() == sah.bvh_digest()
        sc.bvh_validate()
        monkeypatch.delenv("RTAMD_LBVH_MAX_DEPTH")
        assert sc.update_vertices(d003["vertices"], mode="rebuild") == "rebuilt_cluster"
        assert sc.build_info()["fallback"] == "none"
        assert np.array_equal(sc.render(P)[0], d003["frame"])
        assert sc.bvh_digest() == d003["digest"]


def test_fallback_lands_on_the_morton_builder(workdir, monkeypatch, gpu_available):
    import _lbvh_scenes as L
    v, t = L.indexed_grid(workdir)
    with L.create(v, t, builder="lbvh") as lb, L.create(v, t, builder="cluster") as cl:
        limit, digest = lb.bvh_info()["depth"], lb.bvh_digest()
        assert limit < cl.bvh_info()["depth"]   # deeper than the limit allows the clustered tree, not the Morton tree
    with L.create(v, t, device=0, builder="sah") as sah, L.create(v, t, device=0, builder="cluster") as sc:
        want = sah.render(P)[0]
        assert sc.builder == ("cluster", "cluster") and np.array_equal(sc.render(P)[0], want)
        monkeypatch.setenv("RTAMD_LBVH_MAX_DEPTH", str(limit))
        assert sc.update_vertices(v, mode="rebuild") == "rebuilt_lbvh"
        assert sc.builder == ("cluster", "lbvh")
        assert sc.build_info()["fallback"] == "depth" and sc.build_info()["built_with"] == "lbvh"
        assert sc.bvh_digest() == digest
        assert np.array_equal(sc.render(P)[0], want)
        monkeypatch.delenv("RTAMD_LBVH_MAX_DEPTH")
        assert sc.update_vertices(v, mode="rebuild") == "rebuilt_cluster"
        assert np.array_equal(sc.render(P)[0], want)


def test_trace_rays_equal_the_sah_scene(arr, d003):
    rng = np.random.default_rng(9)
    cs = R.default_corners(W, H)
    t = rng.uniform(0, 1, (300, 2)).astype(np.float32)
    o = np.tile(np.array(P.camera_pos, np.float32), (300, 1))
    d = (cs[1] * (1 - t[:, :1]) * (1 - t[:, 1:]) + cs[3] * (1 - t[:, :1]) * t[:, 1:] + cs[5] * t[:, :1] * (1 - t[:, 1:]) +
         cs[7] * t[:, :1] * t[:, 1:]).astype(np.float32)
    with _create(arr, d003["vertices"]) as sc, S.create(arr, d003["vertices"], device=0) as sah:
        rgb, counts = sc.perform_ray_tracing(P, o, d)      # rt_trace_rays
        srgb, scounts = sah.perform_ray_tracing(P, o, d)
        assert np.array_equal(_bits(rgb), _bits(srgb)) and np.array_equal(counts, scounts)
        assert np.count_nonzero(rgb) > 100
