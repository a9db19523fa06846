"""Device-resident ray queries (rt_intersect_mesh_device, rt_occluded_device, rt_trace_rays_device:
k_bvh_query_rays, k_query_rays, k_gen_rays_device): rays in torch CUDA tensors, results in torch CUDA
tensors, on the caller's stream. Closest hits and colours are the host entries' and the oracle's bits;
occlusion is the expectation computed from the oracle's closest hit and the materials.

Scenes, rays and what the oracle alone says about them: tests/_query_scenes.py. Equality is of bytes
throughout, except the traced colour against the oracle (the suite's F32_TOL: specular powf rounding).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _query_scenes as QS
import _refit_scenes as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CAP = 264                      # output rows allocated (more than any n here)
IDX_SENTINEL = -7
NAN_SENTINEL = 0x7FC0DEAD      # a NaN bit pattern no kernel computes
BLK_SENTINEL = 0xEE
F32_TOL = 2e-6                 # the suite's float RGB tolerance (tests/test_gpu_parity.py)
STRIDES = (3, 4)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _dev_rays(o, d, stride):
    """The rays as CUDA tensors in either layout; the padded layout's w holds values that must not matter."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    if stride == 4:
        o = np.concatenate([o, np.full((len(o), 1), 123.0, np.float32)], axis=1)
        d = np.concatenate([d, np.full((len(d), 1), np.nan, np.float32)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(o)).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)


def _sentinel_out():
    idx = torch.full((CAP,), IDX_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((CAP, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    blk = torch.full((CAP,), BLK_SENTINEL, dtype=torch.uint8, device=DEV)
    return idx, pts, blk


def _check_closest(idx, pts, want, live):
    """Rows < live are the wanted index and point bits; later rows still hold the sentinels."""
    idx, pb = _np(idx), _bits(pts)
    assert np.array_equal(idx[:live], want["index"][:live])
    assert np.array_equal(pb[:live], _bits(want["point"][:live]))
    assert (idx[live:] == IDX_SENTINEL).all() and (pb[live:] == NAN_SENTINEL).all()


def _check_blocked(blk, want_blocked, live):
    blk = _np(blk)
    assert np.array_equal(blk[:live], want_blocked[:live])
    assert (blk[live:] == BLK_SENTINEL).all()


def _scene_case(spec, workdir, stem):
    path = scenes.write_sphere_grid(spec, workdir, stem)
    orc = O.OracleScene(path)
    o, d = QS.r200()
    case = dict(path=path, orc=orc, o=o, d=d, **QS.oracle_answers(orc, o, d))
    return case


@pytest.fixture(scope="module")
def q(workdir, gpu_available):
    """Scene Q, R200 and the oracle's answers (computed once), with the conditions that keep a case from
    passing empty."""
    case = _scene_case(QS.SPEC_Q, workdir, "query_q")
    assert orc_counts(case) == 1640
    hit = case["index"] >= 0
    assert hit.sum() >= 100 and (~hit).sum() >= 20 and case["transparent_closest"].sum() >= 10
    for n in (1, 63, 64, 65):
        assert hit[:n].all()
    assert 0 < (~hit[:129]).sum() and len(set(case["index"][hit])) >= 50
    return case


def orc_counts(case):
    return case["orc"].counts()[1]


@pytest.fixture(scope="module")
def qo(workdir, q):
    case = _scene_case(QS.SPEC_QO, workdir, "query_qo")
    assert np.array_equal(case["index"], q["index"])   # the same geometry: only a material differs
    return case


@pytest.fixture(scope="module")
def sc_q(q):
    with R.Scene.load(q["path"], device=0) as sc:
        yield sc


@pytest.fixture(scope="module")
def sc_qo(qo):
    with R.Scene.load(qo["path"], device=0) as sc:
        yield sc


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", QS.PREFIXES)
def test_closest_hit_is_the_oracles_bitwise(q, sc_q, n, stride):
    do, dd = _dev_rays(q["o"][:n], q["d"][:n], stride)
    idx, pts, _ = _sentinel_out()
    ridx, rpts = sc_q.intersect_mesh_device(do, dd, out=(idx, pts))
    assert ridx.shape == (n,) and rpts.shape == (n, 3) and ridx.data_ptr() == idx.data_ptr()
    _check_closest(idx, pts, q, n)
    # ... and rt_intersect_mesh's, with tensors the call allocates
    hidx, hpts = sc_q.intersect_mesh(q["o"][:n], q["d"][:n])
    aidx, apts = sc_q.intersect_mesh_device(do, dd)
    assert aidx.dtype == torch.int32 and apts.dtype == torch.float32 and aidx.device == DEV
    assert np.array_equal(_np(aidx), hidx) and np.array_equal(_bits(apts), _bits(hpts))


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("count,live", [(0, 0), (1, 1), (64, 64), (65, 65), (200, 200), (1000, 200), (-5, 0)])
def test_device_count_decides_the_live_rays(q, sc_q, count, live, stride):
    do, dd = _dev_rays(q["o"], q["d"], stride)
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    idx, pts, blk = _sentinel_out()
    sc_q.intersect_mesh_device(do, dd, count=cnt, out=(idx[:200], pts[:200]))
    sc_q.occluded_device(do, dd, count=cnt, out=blk[:200])
    _check_closest(idx, pts, q, live)
    _check_blocked(blk, q["blocked"], live)
    # no `out`: dead entries are defined (-1, zeros)
    aidx, apts = sc_q.intersect_mesh_device(do, dd, count=cnt)
    ablk = sc_q.occluded_device(do, dd, count=cnt)
    assert (_np(aidx)[live:] == -1).all() and (_bits(apts)[live:] == 0).all() and (_np(ablk)[live:] == 0).all()
    assert np.array_equal(_np(aidx)[:live], q["index"][:live]) and np.array_equal(_np(ablk)[:live], q["blocked"][:live])


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_occlusion_is_the_closest_hits_material(q, qo, sc_q, sc_qo, stride):
    do, dd = _dev_rays(q["o"], q["d"], stride)
    _, _, blk = _sentinel_out()
    sc_q.occluded_device(do, dd, out=blk)
    _check_blocked(blk, q["blocked"], 200)
    tr = q["transparent_closest"]
    assert tr.sum() >= 10 and (_np(blk)[:200][tr] == 0).all()        # the opaque back plane behind them does not block
    assert np.array_equal(_np(blk)[:200][~tr], (q["index"] >= 0)[~tr].astype(np.uint8))
    # every material opaque (the any-hit walk): blocked = some triangle is hit; those rays are 1 there
    _, _, blk_o = _sentinel_out()
    sc_qo.occluded_device(do, dd, out=blk_o)
    assert not qo["transparent_closest"].any()
    _check_blocked(blk_o, (qo["index"] >= 0).astype(np.uint8), 200)
    assert (_np(blk_o)[:200][tr] == 1).all()


# 4 -------------------------------------------------------------------------------------------------
def _all_answers(sc, o, d):
    out = []
    for stride in STRIDES:
        do, dd = _dev_rays(o, d, stride)
        idx, pts = sc.intersect_mesh_device(do, dd)
        blk = sc.occluded_device(do, dd)
        out.append((_np(idx).tobytes(), _bits(pts).tobytes(), _np(blk).tobytes()))
    assert out[0] == out[1]
    return out[0]


@pytest.mark.parametrize("which", ["q", "qo"])
def test_every_traversal_gives_the_same_bytes(q, qo, which):
    case = q if which == "q" else qo
    want = (case["index"].tobytes(), _bits(case["point"]).tobytes(), case["blocked"].tobytes())
    with R.Scene.load(case["path"], device=0) as sc:
        assert sc.accel() == "bvh" and sc.bvh_info()["nodes4"] > 85
        assert _all_answers(sc, case["o"], case["d"]) == want, "width 4"
        sc.tune("bvh_width", 2)
        assert _all_answers(sc, case["o"], case["d"]) == want, "width 2"
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        assert _all_answers(sc, case["o"], case["d"]) == want, "brute force"
        sc.set_accel("bvh")
        v = sc.export()["vertices"]
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(v, "rebuild") == "rebuilt_" + builder
            assert sc.builder == (builder, builder)
            assert _all_answers(sc, case["o"], case["d"]) == want, builder


# 5 -------------------------------------------------------------------------------------------------
def test_query_after_a_device_vertex_update(workdir, gpu_available):
    arr = S.base_arrays(workdir)
    new = S.deform(arr["vertices"], 0.03)
    orc = S.oracle_scene(arr, new, workdir, "dq_d003")
    # the rays of test_refit_frames_and_queries_equal_fresh_and_oracle: over the frame and at the sliver
    rng = np.random.default_rng(5)
    cs = R.default_corners(S.W, S.H)
    t = rng.uniform(0, 1, (200, 2)).astype(np.float32)
    o = np.tile(np.array((0.0, 0.0, 4.0), np.float32), (200, 1))
    d = (cs[1] * (1 - t[:, :1]) * (1 - t[:, 1:]) + cs[3] * (1 - t[:, :1]) * t[:, 1:] + cs[5] * t[:, :1] * (1 - t[:, 1:]) +
         cs[7] * t[:, :1] * t[:, 1:]).astype(np.float32)
    sliver = new[arr["n_grid_vertices"]:arr["n_grid_vertices"] + 3]
    d[:20] = (sliver[0] + (sliver[1] - sliver[0]) * t[:20, :1] + (sliver[2] - sliver[1]) * t[:20, :1] * t[:20, 1:]).astype(np.float32)
    want = QS.oracle_answers(orc, o, d)
    assert (want["index"] == 1640).sum() > 0 and (want["index"] >= 0).sum() > 50
    with S.create(arr, device=0) as sc:
        assert sc.update_vertices(torch.from_numpy(new).to(DEV)) == "refit"
        for stride in STRIDES:
            do, dd = _dev_rays(o, d, stride)
            idx, pts, blk = _sentinel_out()
            sc.intersect_mesh_device(do, dd, out=(idx, pts))
            sc.occluded_device(do, dd, out=blk)
            _check_closest(idx, pts, want, 200)
            _check_blocked(blk, want["blocked"], 200)


# 6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_triangle", "two_slivers"])
def test_tiny_trees(name, gpu_available):
    v, t, _ = S.tiny_scenes()[name]
    g = np.linspace(-1.2, 1.2, 9, dtype=np.float32)
    gx, gy = np.meshgrid(g, g)
    o = np.stack([gx.ravel(), gy.ravel(), np.full(81, 2.0, np.float32)], axis=1).astype(np.float32)
    d = np.stack([gx.ravel(), gy.ravel(), np.full(81, -1.0, np.float32)], axis=1).astype(np.float32)
    cen = v[t.astype(np.int64)].mean(axis=1).astype(np.float32)              # through each triangle's centroid
    o = np.concatenate([o, cen + np.array([0.1, -0.2, 3.0], np.float32)]).astype(np.float32)
    d = np.concatenate([d, cen]).astype(np.float32)
    with R.Scene.create(v, t, np.zeros(len(t), np.uint32), S.TINY_MATERIALS, device=0) as sc:
        hidx, hpts = sc.intersect_mesh(o, d)
        assert (hidx >= 0).sum() > 0 and (hidx < 0).sum() > 0          # rays through and past
        want = dict(index=hidx, point=hpts)
        for stride in STRIDES:
            do, dd = _dev_rays(o, d, stride)
            idx, pts, blk = _sentinel_out()
            sc.intersect_mesh_device(do, dd, out=(idx, pts))
            sc.occluded_device(do, dd, out=blk)
            _check_closest(idx, pts, want, len(o))
            _check_blocked(blk, (hidx >= 0).astype(np.uint8), len(o))     # (the material is opaque)


# 7 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(q, workdir):
    st = torch.cuda.Stream(device=DEV)
    ho, hd = torch.from_numpy(q["o"]).pin_memory(), torch.from_numpy(q["d"]).pin_memory()
    with R.Scene.load(q["path"], device=0) as sc:
        with torch.cuda.stream(st):
            do = ho.to(DEV, non_blocking=True) * 1.0
            dd = hd.to(DEV, non_blocking=True) * 1.0
            idx, pts = sc.intersect_mesh_device(do, dd)                 # (the current stream: st)
            blk = sc.occluded_device(do, dd, stream=st)
            hidx, hpts, hblk = (x.to("cpu", non_blocking=True) for x in (idx, pts, blk))
        st.synchronize()
        assert np.array_equal(hidx.numpy(), q["index"]) and np.array_equal(_bits(hpts.numpy()), _bits(q["point"]))
        assert np.array_equal(hblk.numpy(), q["blocked"])
        # a query in flight when the vertices move answers for the old vertices; the next one for the new
        e = sc.export()
        arr = dict(vertices=e["vertices"], triangles=e["triangles"], tri_mat=e["tri_mat"], materials=e["materials"],
                   mtl=q["path"][:-4] + ".mtl")
        new = S.deform(e["vertices"], 0.03)
        moved = QS.oracle_answers(S.oracle_scene(arr, new, workdir, "dq_q_moved"), q["o"], q["d"])
        assert not np.array_equal(_bits(moved["point"]), _bits(q["point"]))
        reps = 512
        with torch.cuda.stream(st):
            bo, bd = do.repeat(reps, 1), dd.repeat(reps, 1)
            idx, pts = sc.intersect_mesh_device(bo, bd)
            blk = sc.occluded_device(bo, bd)
        assert sc.update_vertices(new) == "refit"
        with torch.cuda.stream(st):
            idx2, pts2 = sc.intersect_mesh_device(do, dd)
            blk2 = sc.occluded_device(do, dd)
        st.synchronize()
        assert np.array_equal(_np(idx).reshape(reps, 200), np.tile(q["index"], (reps, 1)))
        assert np.array_equal(_bits(pts).reshape(reps, 200, 3), np.tile(_bits(q["point"]), (reps, 1, 1)))
        assert np.array_equal(_np(blk).reshape(reps, 200), np.tile(q["blocked"], (reps, 1)))
        assert np.array_equal(_np(idx2), moved["index"]) and np.array_equal(_bits(pts2), _bits(moved["point"]))
        assert np.array_equal(_np(blk2), moved["blocked"])


# 8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_traced_colour_is_the_host_entrys(q, sc_q, stride):
    P = R.RenderParams(width=S.W, height=S.H, pf=1, max_lvl=3, lights=S.LIGHTS)
    OP = O.make_params(S.W, S.H, pf=1, max_lvl=3, lights=S.LIGHTS)
    oracle_rgb = np.array([q["orc"].trace(OP, q["o"][i], q["d"][i])[0] for i in range(200)], np.float32)
    for n in (1, 65, 200):
        hrgb, hcounts = sc_q.perform_ray_tracing(P, q["o"][:n], q["d"][:n])
        do, dd = _dev_rays(q["o"][:n], q["d"][:n], stride)
        out = torch.full((CAP, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        rgb, counts = sc_q.perform_ray_tracing_device(P, do, dd, out=out, want_counts=True)
        assert rgb.shape == (n, 3)
        assert np.array_equal(_bits(out)[:n], _bits(hrgb)) and (_bits(out)[n:] == NAN_SENTINEL).all()
        assert [int(c) for c in counts] == [int(c) for c in hcounts] and int(counts[0]) == n
        assert np.abs(_np(rgb) - oracle_rgb[:n]).max() <= F32_TOL
        rgb2 = sc_q.perform_ray_tracing_device(P, do, dd)      # no counts: stream-ordered, read after torch's sync
        assert np.array_equal(_bits(rgb2), _bits(hrgb))
    assert len(np.unique(_bits(hrgb), axis=0)) > 50           # colours with something in them


# 9 -------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(q, sc_q):
    L = _capi.lib()
    do, dd = _dev_rays(q["o"][:8], q["d"][:8], 4)
    idx, pts, blk = _sentinel_out()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    h = sc_q.handle
    assert L.rt_intersect_mesh_device(h, vp(do), vp(dd), 4, -1, None, vp(idx), vp(pts), None) == _capi.RT_E_ARG
    assert L.rt_intersect_mesh_device(h, vp(do), vp(dd), 5, 8, None, vp(idx), vp(pts), None) == _capi.RT_E_ARG
    assert L.rt_intersect_mesh_device(h, vp(do, 4), vp(dd), 4, 7, None, vp(idx), vp(pts), None) == _capi.RT_E_ARG   # 16-B rule
    assert L.rt_intersect_mesh_device(h, vp(do), vp(dd), 3, 8, None, vp(idx, 2), vp(pts), None) == _capi.RT_E_ARG
    assert L.rt_intersect_mesh_device(h, vp(do), None, 4, 8, None, vp(idx), vp(pts), None) == _capi.RT_E_ARG
    assert L.rt_occluded_device(h, vp(do), vp(dd), 4, 8, None, None, None) == _capi.RT_E_ARG
    assert L.rt_occluded_device(h, vp(do), vp(dd), 4, 8, vp(idx, 1), vp(blk), None) == _capi.RT_E_ARG
    assert L.rt_intersect_mesh_device(h, None, None, 3, 0, None, None, None, None) == _capi.RT_OK    # n == 0: nothing to do
    torch.cuda.synchronize()
    assert (_np(idx) == IDX_SENTINEL).all() and (_np(blk) == BLK_SENTINEL).all()   # nothing was enqueued
    # the Python forms: the wrong device's count, an `out` too small, mismatched shapes
    with pytest.raises(ValueError):
        sc_q.intersect_mesh_device(do, dd, count=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        sc_q.occluded_device(do, dd, out=blk[:4])
    with pytest.raises(ValueError):
        sc_q.intersect_mesh_device(do, dd[:4])
    e_idx, e_pts = sc_q.intersect_mesh_device(do[:0], dd[:0])
    assert e_idx.shape == (0,) and e_pts.shape == (0, 3)
