"""Closest-point queries (rt_closest_point_device, rt_closest_point: k_bvh_point_query, k_point_query): the
nearest point of the mesh per query point as {triangle, distance, s, t} records, points and results in torch
CUDA tensors.

The expectation is tests/_closest_point_ref.py, the numpy restatement that tests/test_closest_point_ref.py
checks on the CPU (and whose counts say that no case below passes empty). Equality is of bytes throughout: there
is no tolerance. Scenes: Q (tests/_query_scenes.py), shingles (tests/_edge_rays.py), "far tiny" (triangles of a
few ulps near 2^10 next to a handful at the origin), one triangle, an empty mesh, an all-degenerate mesh, and
the refit scene S (tests/_refit_scenes.py: a sliver on the always list and a zero-area triangle).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _closest_point_ref as CP
import _query_scenes as QS
import _range_ref as RR
import _refit_scenes as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
REC_SENTINEL = -7
NAN_SENTINEL = 0x7FC0DEAD      # a NaN bit pattern no kernel computes
STRIDES = (3, 4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = np.array([0xFFFFFFFF, CP.INF_BITS, 0, 0], np.uint32)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _dev_points(p, stride):
    """The points as a CUDA tensor in either layout; the padded layout's w holds values that must not matter."""
    p = np.asarray(p, F32)
    if stride == 4:
        w = np.where(np.arange(len(p)) % 2 == 0, np.nan, 123.0).astype(F32)[:, None]
        p = np.concatenate([p, w], axis=1)
    return torch.from_numpy(np.ascontiguousarray(p)).to(DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


class Case:
    """Triangles, points, and every point x triangle pair by the helper (computed once, never changed)."""

    def __init__(self, T, p, path=None):
        self.path, self.T, self.p = path, np.ascontiguousarray(T, F32), p
        self.P = CP.pairs(p, self.T)
        for a in self.P.values():
            a.setflags(write=False)
        self.want = CP.closest(self.P)

    def closest(self, rmax=None):
        return CP.closest(self.P, rmax)


def _file_case(path, seed, surface=None):
    T = RR.scene_triangles(O.OracleScene(path))[0]
    return Case(T, CP.points_for(T, seed, surface=None if surface is None else surface(T)), path)


@pytest.fixture(scope="module")
def q(workdir, gpu_available):
    return _file_case(scenes.write_sphere_grid(QS.SPEC_Q, workdir, "cp_q"), 101, CP.q_surface_points)


@pytest.fixture(scope="module")
def shingles(workdir, gpu_available):
    return _file_case(CP.write_obj(workdir, "cp_shingles", CP.shingles_triangles()), 102)


@pytest.fixture(scope="module")
def far(workdir, gpu_available):
    return _file_case(CP.write_obj(workdir, "cp_far", CP.far_tiny_triangles()), 103)


@pytest.fixture(scope="module")
def one(workdir, gpu_available):
    return _file_case(CP.write_obj(workdir, "cp_one", CP.one_triangle()), 104)


def _query(sc, p, stride=3, rmax=None, count=None, n=None, want_points=True, stream=None):
    """One query into sentinel-filled outputs: (records [cap, 4] uint32, point bits [cap, 3])."""
    n = len(p) if n is None else n
    cap = len(p) + 8
    dp = _dev_points(p[:n], stride)
    rec = torch.full((cap, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((cap, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    res = sc.closest_point_device(dp, rmax=_dev(None if rmax is None else rmax[:n]), count=count, out=(rec, pts) if want_points else rec,
                                  want_points=want_points, stream=stream)
    assert len(res) == (4 if want_points else 3) and res[0].shape == (n,) and res[1].shape == (n,) and res[2].shape == (n, 2)
    assert res[0].data_ptr() == rec.data_ptr() and res[0].dtype == torch.int32 and res[1].dtype == res[2].dtype == torch.float32
    return _np(rec).view(np.uint32), _bits(pts)


def _check(got, want, live, what="", points=True):
    rec, pts = got
    bad = np.flatnonzero((rec[:live] != want["record"][:live]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} records differ, first points {bad[:5]}: {rec[bad[:5]]} for {want['record'][bad[:5]]}"
    if points:
        assert np.array_equal(pts[:live], _bits(want["point"][:live])), f"{what}: points differ"
    else:
        assert (pts == NAN_SENTINEL).all(), f"{what}: points written without want_points"
    assert (rec[live:].view(np.int32) == REC_SENTINEL).all() and (pts[live:] == NAN_SENTINEL).all(), f"{what}: rows past {live} written"


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles", "far", "one"])
def test_scenes_against_the_restatement(which, request):
    case = request.getfixturevalue(which)
    n = len(case.p)
    hit = case.want["triangle"] >= 0
    assert 240 <= hit.sum() <= n - 11 and (case.want["record"][~hit] == MISS).all()
    with R.Scene.load(case.path, device=0) as sc:
        sc.bvh_validate()
        for stride in STRIDES:
            _check(_query(sc, case.p, stride), case.want, n, f"{which}, stride {stride}")
            _check(_query(sc, case.p, stride, want_points=False), case.want, n, f"{which}, stride {stride}, no points", points=False)
        # the views of tensors the call allocates
        tri, dist, st, pts = sc.closest_point_device(_dev_points(case.p, 3), want_points=True)
        assert tri.dtype == torch.int32 and dist.dtype == st.dtype == torch.float32 and st.shape == (n, 2) and pts.shape == (n, 3)
        assert np.array_equal(_np(tri), case.want["triangle"]) and np.array_equal(_bits(dist), case.want["record"][:, 1])
        assert np.array_equal(_bits(st), case.want["record"][:, 2:]) and np.array_equal(_bits(pts), _bits(case.want["point"]))
        # the closest point is the record's V0 + s (V1 - V0) + t (V2 - V0) up to rounding, at the record's distance
        k = case.want["triangle"][hit]
        T64, s, t = case.T[k].astype(np.float64), _np(st)[hit, 0:1].astype(np.float64), _np(st)[hit, 1:2].astype(np.float64)
        c = T64[:, 0] + s * (T64[:, 1] - T64[:, 0]) + t * (T64[:, 2] - T64[:, 0])
        scale = CP.scene_m1(case.T) + np.abs(case.p[hit].astype(np.float64)).sum(axis=1)
        assert (np.abs(c - _np(pts)[hit]).sum(axis=1) <= 16 * 2.0 ** -24 * scale).all()
        assert (np.abs(np.linalg.norm(case.p[hit] - c, axis=1) - _np(dist)[hit]) <= 16 * 2.0 ** -24 * scale).all()
        # the host entry: the device entry's bytes
        htri, hdist, hst, hpts = sc.closest_point(case.p)
        assert np.array_equal(htri, case.want["triangle"]) and np.array_equal(_bits(hdist), case.want["record"][:, 1])
        assert np.array_equal(_bits(hst), case.want["record"][:, 2:]) and np.array_equal(_bits(hpts), _bits(case.want["point"]))


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles", "far"])
def test_every_walk_and_builder_gives_the_same_bytes(which, request):
    case = request.getfixturevalue(which)
    n = len(case.p)
    with R.Scene.load(case.path, device=0) as sc:
        def run(what, stride=4):
            _check(_query(sc, case.p, stride), case.want, n, f"{which}, {what}")

        run("four-wide")
        sc.tune("lds_stack", 1)                                 # every push beyond the first through the overflow path
        run("four-wide, lds_stack 1")
        sc.tune("lds_stack", 16)
        sc.set_profiling(True, count_work=True)                 # the counting instantiations
        sc.reset_stats()
        run("four-wide, counting", 3)
        tests, visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
        assert tests > 0 and visits > 0
        sc.tune("bvh_width", 2)
        run("binary, counting")
        sc.set_profiling(False)
        run("binary", 3)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        run("brute force", 3)
        run("brute force", 4)
        sc.set_accel("bvh")
        v = sc.export()["vertices"]
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(v, "rebuild") == "rebuilt_" + builder
            sc.bvh_validate()
            for width in (4, 2):
                sc.tune("bvh_width", width)
                run(f"{builder}, width {width}")


# 3 -------------------------------------------------------------------------------------------------
def test_far_tiny_walks_equal_brute_force_near_the_triangles(far):
    """4,096 points within a few edge lengths of triangles of a few ulps at 2^10: the computed closest point is
    rounded at the magnitude of the coordinates and can lie outside a triangle's box, so a box bound that is not
    deflated culls the winner. Every tree against the loop over all triangles."""
    p = CP.near_far_points(far.T)
    with R.Scene.load(far.path, device=0) as sc:
        sc.set_accel("brute_force")
        ref = _query(sc, p, 3)
        tri = ref[0][:len(p), 0].view(np.int32)
        assert (tri >= 0).all() and (tri < CP.N_FAR).all() and len(np.unique(tri)) >= 100
        small = ref[0][:len(p), 1].view(F32) <= 8 * CP.FAR_ULP
        assert small.sum() >= 1000                               # distances of the size of the rounding of c
        sc.set_accel("bvh")
        v = sc.export()["vertices"]
        for builder in ("sah", "lbvh", "cluster"):
            sc.set_builder(builder)
            sc.update_vertices(v, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                got = _query(sc, p, 4)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), f"{builder}, width {width}"


# 4 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "far"])
def test_radius_menu(which, request):
    case = request.getfixturevalue(which)
    n = len(case.p)
    dist = case.want["distance"]
    hit = case.want["triangle"] >= 0
    menu = {
        "twice the distance": (F32(2) * dist).astype(F32),
        "half the distance": (F32(0.5) * dist).astype(F32),
        "the distance": dist,
        "just above the distance": np.nextafter(dist, F32(np.inf)).astype(F32),
        "zero": np.zeros(n, F32),
        "negative": np.full(n, -1.0, F32),
        "nan": np.full(n, np.nan, F32),
        "+inf": np.full(n, np.inf, F32),
        "mixed": np.where(np.arange(n) % 3 == 0, F32(np.nan), np.where(np.arange(n) % 3 == 1, F32(0.05), F32(np.inf))).astype(F32),
    }
    with R.Scene.load(case.path, device=0) as sc:
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            for name, rmax in menu.items():
                want = case.closest(rmax)
                _check(_query(sc, case.p, 3 if accel == "bvh" else 4, rmax=rmax), want, n, f"{which}, {accel}, rmax {name}")
                got = (want["triangle"] >= 0).sum()
                if name in ("half the distance", "zero", "negative", "nan"):
                    assert (want["triangle"][dist > 0] == -1).all(), name
                elif name in ("twice the distance", "+inf"):
                    assert got == (hit & ((dist > 0) | (name == "+inf"))).sum(), name
                elif name == "the distance" and which == "q":
                    assert 10 <= got <= hit.sum() - 10, name          # rmax * rmax falls on either side of dist2
        sc.set_accel("bvh")
        htri = sc.closest_point(case.p, rmax=menu["mixed"])[0]
        assert np.array_equal(htri, case.closest(menu["mixed"])["triangle"])


# 5 -------------------------------------------------------------------------------------------------
def test_counts_and_sentinels(q):
    with R.Scene.load(q.path, device=0) as sc:
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            for n in (1, 63, 64, 65, 257):
                _check(_query(sc, q.p, 3, n=n), q.want, n, f"{accel}, n {n}")
                for c in (n - 1, n, n + 5, 0, -3):
                    live = min(max(c, 0), n)
                    cnt = torch.tensor([c], dtype=torch.int32, device=DEV)
                    _check(_query(sc, q.p, 4, n=n, count=cnt), q.want, live, f"{accel}, n {n}, count {c}")
        sc.set_accel("bvh")
        # rows a device count leaves unwritten in tensors the call allocates are the miss record
        cnt = torch.tensor([40], dtype=torch.int32, device=DEV)
        tri, dist, st, pts = sc.closest_point_device(_dev_points(q.p[:65], 3), count=cnt, want_points=True)
        assert np.array_equal(_np(tri)[:40], q.want["triangle"][:40]) and (_np(tri)[40:] == -1).all()
        assert np.isinf(_np(dist)[40:]).all() and (_np(st)[40:] == 0).all() and (_np(pts)[40:] == 0).all()
        # n == 0
        tri, dist, st = sc.closest_point_device(torch.zeros((0, 3), dtype=torch.float32, device=DEV))
        assert tri.shape == (0,) and st.shape == (0, 2)
        assert sc.closest_point(np.zeros((0, 3), F32))[0].shape == (0,)


# 6 -------------------------------------------------------------------------------------------------
def test_empty_and_degenerate_meshes(one, workdir):
    p = one.p
    n = len(p)
    miss = dict(record=np.tile(MISS, (n, 1)), point=np.zeros((n, 3), F32))
    deg = CP.degenerate_triangles()
    with R.Scene.load(CP.write_obj(workdir, "cp_degenerate", deg), device=0) as sc:
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            for stride in STRIDES:
                _check(_query(sc, p, stride), miss, n, f"degenerate, {accel}")
    with R.Scene.load(one.path, device=0) as sc:
        _check(_query(sc, p, 3), one.want, n, "one triangle")
        sc.set_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32))
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            _check(_query(sc, p, 4), miss, n, f"empty, {accel}")
        sc.set_accel("bvh")
        v = deg.reshape(-1, 3)
        sc.set_mesh(v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3), np.zeros(len(deg), np.uint32))
        _check(_query(sc, p, 3), miss, n, "degenerate through set_mesh")
        v = one.T.reshape(-1, 3)
        sc.set_mesh(v, np.arange(3, dtype=np.uint32).reshape(1, 3), np.zeros(1, np.uint32))
        _check(_query(sc, p, 3), one.want, n, "one triangle again")


# 7 -------------------------------------------------------------------------------------------------
def test_always_list_and_never_class_after_refit_and_set_mesh(q, shingles, workdir):
    """Scene S holds a sliver (tested for every point) and a zero-area triangle (no candidate). After a refit on
    the device and after set_mesh_device the answers are those of the restatement on the new triangles, which
    are a freshly created scene's."""
    arr = S.base_arrays(workdir)
    tri_idx = arr["triangles"].astype(np.int64)
    T0 = arr["vertices"][tri_idx]
    p = CP.points_for(T0, 106)
    near = np.array([[0.5, 0.002, 1.0], [0.9, 0.01, 1.02], [0.2, -0.01, 0.99]], F32)      # next to the sliver
    p = np.ascontiguousarray(np.concatenate([p, near]), F32)
    n = len(p)
    before = Case(T0, p)
    assert not before.P["candidate"][0, -1] and before.P["candidate"][0, :-1].all()
    assert (before.want["triangle"][-3:] == len(T0) - 2).all()                              # the sliver wins there
    new = S.deform(arr["vertices"], 0.03)
    after = Case(new[tri_idx], p)
    assert not np.array_equal(after.want["record"], before.want["record"])
    with S.create(arr, device=0) as sc:
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _check(_query(sc, p, 3), before.want, n, f"S, width {width}")
        sc.tune("bvh_width", 4)
        assert sc.update_vertices(torch.from_numpy(new).to(DEV)) == "refit"
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _check(_query(sc, p, 4), after.want, n, f"S after the refit, width {width}")
        with S.create(arr, vertices=new, device=0) as fresh:
            a, b = _query(fresh, p, 3), _query(sc, p, 3)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # another mesh altogether, from device tensors: the shingles, then answers for the shingles' points
        v = torch.from_numpy(np.ascontiguousarray(shingles.T.reshape(-1, 3))).to(DEV)
        t = torch.arange(3 * len(shingles.T), dtype=torch.int32, device=DEV).reshape(-1, 3)
        m = torch.zeros(len(shingles.T), dtype=torch.int32, device=DEV)
        sc.set_mesh(v, t, m)
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _check(_query(sc, shingles.p, 3), shingles.want, len(shingles.p), f"after set_mesh_device, width {width}")


# 8 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(q):
    """A query queued before update_vertices answers for the old vertices, one queued after it for the new; on a
    stream that is not the default."""
    st = torch.cuda.Stream(device=DEV)
    reps, n = 16, len(q.p)
    with R.Scene.load(q.path, device=0) as sc:
        e = sc.export()
        new = S.deform(e["vertices"], 0.03)
        moved = Case(new[e["triangles"].astype(np.int64)], q.p)
        assert not np.array_equal(moved.want["record"], q.want["record"])
        with torch.cuda.stream(st):
            dp = _dev_points(q.p, 3)
            tri, dist, sts, pts = sc.closest_point_device(dp.repeat(reps, 1), want_points=True)     # (the current stream: st)
        assert sc.update_vertices(new) == "refit"
        with torch.cuda.stream(st):
            tri2, dist2, sts2, pts2 = sc.closest_point_device(dp, want_points=True, stream=st)
        st.synchronize()
        assert np.array_equal(_np(tri).reshape(reps, n), np.tile(q.want["triangle"], (reps, 1)))
        assert np.array_equal(_bits(dist).reshape(reps, n), np.tile(q.want["record"][:, 1], (reps, 1)))
        assert np.array_equal(_bits(sts).reshape(reps, n, 2), np.tile(q.want["record"][:, 2:], (reps, 1, 1)))
        assert np.array_equal(_bits(pts).reshape(reps, n, 3), np.tile(_bits(q.want["point"]), (reps, 1, 1)))
        assert np.array_equal(_np(tri2), moved.want["triangle"]) and np.array_equal(_bits(dist2), moved.want["record"][:, 1])
        assert np.array_equal(_bits(sts2), moved.want["record"][:, 2:]) and np.array_equal(_bits(pts2), _bits(moved.want["point"]))


# 9 -------------------------------------------------------------------------------------------------
def test_the_walk_culls(q):
    """With RT_PROFILE_WORK the point-triangle evaluations per point on scene Q, for 256 points uniform in the
    scene's box, are strictly below the triangle count (the loop over all triangles evaluates every one), and at
    most 1.25 x what profiles/closest_point_probe.json records for each builder (the count is deterministic per
    tree; the margin covers later changes of tree shape only)."""
    with open(os.path.join(ROOT, "profiles", "closest_point_probe.json")) as f:
        measured = json.load(f)["scene_q_work"]
    p = CP.in_box_points(q.T)
    nt = len(q.T)
    assert measured["triangles"] == nt and measured["points"] == len(p)
    want = CP.closest(CP.pairs(p, q.T))
    with R.Scene.load(q.path, device=0) as sc:
        v = sc.export()["vertices"]
        sc.set_profiling(True, count_work=True)
        for builder in ("sah", "lbvh", "cluster"):
            sc.set_builder(builder)
            sc.update_vertices(v, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                sc.reset_stats()
                _check(_query(sc, p, 3), want, len(p), f"{builder}, width {width}")
                tests, visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                per_point = tests / len(p)
                pinned = measured[builder][f"width{width}"]["evaluations_per_point"]
                print(f"{builder} width {width}: {per_point:.3f} evaluations, {visits / len(p):.3f} node visits per point (recorded {pinned})")
                assert 0 < per_point < nt
                assert per_point <= 1.25 * pinned, f"{builder}, width {width}"
        sc.set_profiling(False)


# 10 ------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(q):
    """Each RT_E_ARG case alone on a scene with a device; nothing is written."""
    L = _capi.lib()
    dp = _dev_points(q.p[:8], 4)
    rec = torch.full((16, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((16, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    rb = torch.ones(16, dtype=torch.float32, device=DEV)
    cnt = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with R.Scene.load(q.path, device=0) as sc:
        good = dict(p=vp(dp), stride=4, n=8, count=vp(cnt), rmax=vp(rb), flags=0, out=vp(rec), out2=vp(pts))

        def call(**kw):
            a = dict(good, **kw)
            return L.rt_closest_point_device(sc.handle, a["p"], a["stride"], a["n"], a["count"], a["rmax"], a["flags"], a["out"], a["out2"], None)

        cases = [dict(n=-1), dict(stride=5), dict(stride=0), dict(p=None), dict(p=vp(dp, 4), n=7), dict(stride=3, p=vp(dp, 2)),
                 dict(count=vp(cnt, 2)), dict(rmax=vp(rb, 1)), dict(flags=1), dict(flags=1 << 31), dict(flags=_capi.RANGE_TO_DEST),
                 dict(out=None), dict(out=vp(rec, 8)), dict(out=vp(rec, 4)), dict(out2=vp(pts, 2))]
        for kw in cases:
            assert call(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        assert call(n=0, p=None, out=None, out2=None) == _capi.RT_OK          # n == 0: nothing to do
        torch.cuda.synchronize()
        assert (_np(rec) == REC_SENTINEL).all() and (_bits(pts) == NAN_SENTINEL).all()   # nothing was written
        assert call() == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(rec)[:8] != REC_SENTINEL).all() and (_np(rec)[8:] == REC_SENTINEL).all()
        with pytest.raises(ValueError):
            sc.closest_point_device(dp, rmax=torch.ones(4, dtype=torch.float32, device=DEV))
        with pytest.raises(ValueError):
            sc.closest_point_device(dp, out=torch.zeros((4, 4), dtype=torch.int32, device=DEV))
        with pytest.raises(ValueError):
            sc.closest_point_device(dp, want_points=True, out=rec)
