"""Nearest-triangle queries (rt_nearest_triangles_device, rt_within_radius_device: k_bvh_near_query,
k_point_list_query, k_point_any_query): per query point the k nearest candidate triangles inside its radius as
{triangle, distance, s, t} rows in (dist2, index) order, or only whether there is one; points and results in torch
CUDA tensors.

The expectation is tests/_nearest_ref.py, built on the closest-point restatement, which tests/test_nearest_ref.py
checks on the CPU (and whose counts say that no case below passes empty: lists cut by k, lists shorter than k, ties
cut by the list's end). Equality is of bytes throughout: there is no tolerance. Scenes and points are those of
tests/test_gpu_closest_point.py: Q, shingles, "far tiny", one triangle, an empty mesh, an all-degenerate mesh, and
the refit scene S (a sliver on the always list and a zero-area triangle).
"""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _closest_point_ref as CP
import _nearest_ref as NR
import _query_scenes as QS
import _range_ref as RR
import _refit_scenes as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
REC_SENTINEL = -7
NF_SENTINEL = -9
W_SENTINEL = 0xAB
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
    """Triangles, points, every point x triangle pair by the helper (computed once, never changed), and the
    expectations made from them, each computed once."""

    def __init__(self, T, p, path=None):
        self.path, self.T, self.p = path, np.ascontiguousarray(T, F32), p
        self.P = CP.pairs(p, self.T)
        for a in self.P.values():
            a.setflags(write=False)
        n = len(p)
        self.radii = {"none": None, "0.05": np.full(n, 0.05, F32), "twice": NR.twice_closest(self.P)}
        self._want = {}

    def want(self, k, radius="none"):
        if (k, radius) not in self._want:
            w = NR.nearest(self.P, k, self.radii[radius])
            for a in w.values():
                a.setflags(write=False)
            self._want[k, radius] = w
        return self._want[k, radius]


def _file_case(path, seed, surface=None):
    T = RR.scene_triangles(O.OracleScene(path))[0]
    return Case(T, CP.points_for(T, seed, surface=None if surface is None else surface(T)), path)


@pytest.fixture(scope="module")
def q(workdir, gpu_available):
    return _file_case(scenes.write_sphere_grid(QS.SPEC_Q, workdir, "near_q"), 101, CP.q_surface_points)


@pytest.fixture(scope="module")
def shingles(workdir, gpu_available):
    return _file_case(CP.write_obj(workdir, "near_shingles", CP.shingles_triangles()), 102)


@pytest.fixture(scope="module")
def far(workdir, gpu_available):
    return _file_case(CP.write_obj(workdir, "near_far", CP.far_tiny_triangles()), 103)


@pytest.fixture(scope="module")
def one(workdir, gpu_available):
    return _file_case(CP.write_obj(workdir, "near_one", CP.one_triangle()), 104)


@pytest.fixture(scope="module")
def s_scene(workdir, gpu_available):
    """Scene S's arrays, and its points: points_for plus three next to the sliver."""
    arr = S.base_arrays(workdir)
    T0 = arr["vertices"][arr["triangles"].astype(np.int64)]
    near = np.array([[0.5, 0.002, 1.0], [0.9, 0.01, 1.02], [0.2, -0.01, 0.99]], F32)
    p = np.ascontiguousarray(np.concatenate([CP.points_for(T0, 106), near]), F32)
    return arr, Case(T0, p)


def _open(case, request):
    """A device scene for a case: from its file, or scene S from its arrays."""
    if case.path is not None:
        return R.Scene.load(case.path, device=0)
    return S.create(request.getfixturevalue("s_scene")[0], device=0)


def _query(sc, p, k, stride=3, rmax=None, count=None, n=None, want_points=True, count_all=False, stream=None):
    """One list query into sentinel-filled outputs: (records [cap, k, 4] uint32, nfound [cap], point bits [cap, k, 3])."""
    n = len(p) if n is None else n
    cap = len(p) + 8
    dp = _dev_points(p[:n], stride)
    rec = torch.full((cap, k, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    nf = torch.full((cap,), NF_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((cap, k, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    res = sc.nearest_triangles_device(dp, k, rmax=_dev(None if rmax is None else rmax[:n]), count_all=count_all, count=count,
                                      out=(rec, nf, pts) if want_points else (rec, nf), want_points=want_points, stream=stream)
    assert len(res) == (5 if want_points else 4)
    assert res[0].shape == (n, k) and res[1].shape == (n, k) and res[2].shape == (n, k, 2) and res[3].shape == (n,)
    assert res[0].data_ptr() == rec.data_ptr() and res[0].dtype == torch.int32 and res[1].dtype == res[2].dtype == torch.float32
    assert res[3].data_ptr() == nf.data_ptr() and res[3].dtype == torch.int32
    if want_points:
        assert res[4].shape == (n, k, 3) and res[4].data_ptr() == pts.data_ptr()
    return _np(rec).view(np.uint32), _np(nf), _bits(pts)


def _check(got, want, live, what="", points=True, count_all=False):
    rec, nf, pts = got
    bad = np.flatnonzero((rec[:live] != want["record"][:live]).any(axis=(1, 2)))
    assert bad.size == 0, f"{what}: the rows of {bad.size} points differ, first points {bad[:5]}: {rec[bad[:2]]} for {want['record'][bad[:2]]}"
    wn = want["m" if count_all else "nfound"][:live]
    assert np.array_equal(nf[:live], wn), f"{what}: counts differ at {np.flatnonzero(nf[:live] != wn)[:5]}"
    if points:
        assert np.array_equal(pts[:live], _bits(want["point"][:live])), f"{what}: points differ"
    else:
        assert (pts == NAN_SENTINEL).all(), f"{what}: points written without want_points"
    assert (rec[live:].view(np.int32) == REC_SENTINEL).all() and (nf[live:] == NF_SENTINEL).all() and (pts[live:] == NAN_SENTINEL).all(), \
        f"{what}: rows past {live} written"


def _within(sc, p, stride=3, rmax=None, count=None, n=None, stream=None):
    """One verdict query into a sentinel-filled output [cap] uint8."""
    n = len(p) if n is None else n
    out = torch.full((len(p) + 8,), W_SENTINEL, dtype=torch.uint8, device=DEV)
    res = sc.within_radius_device(_dev_points(p[:n], stride), rmax=_dev(None if rmax is None else rmax[:n]), count=count, out=out,
                                  stream=stream)
    assert res.shape == (n,) and res.dtype == torch.uint8 and res.data_ptr() == out.data_ptr()
    return _np(out)


def _check_within(got, want, live, what=""):
    assert np.array_equal(got[:live], want[:live]), f"{what}: verdicts differ at {np.flatnonzero(got[:live] != want[:live])[:5]}"
    assert (got[live:] == W_SENTINEL).all(), f"{what}: verdicts past {live} written"


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles", "far", "one", "s"])
def test_scenes_against_the_restatement(which, request):
    case = request.getfixturevalue("s_scene")[1] if which == "s" else request.getfixturevalue(which)
    n = len(case.p)
    with _open(case, request) as sc:
        sc.bvh_validate()
        for radius in ("none", "0.05", "twice"):
            rmax = case.radii[radius]
            for k in NR.KS:
                want = case.want(k, radius)
                off = None
                for stride, want_points, count_all in itertools.product(STRIDES, (True, False), (False, True)):
                    what = f"{which}, rmax {radius}, k {k}, stride {stride}, points {want_points}, count_all {count_all}"
                    got = _query(sc, case.p, k, stride, rmax=rmax, want_points=want_points, count_all=count_all)
                    _check(got, want, n, what, points=want_points, count_all=count_all)
                    if not count_all:
                        off = got[0]
                    else:
                        assert np.array_equal(got[0], off), f"{what}: the rows differ with the flag"
            _check_within(_within(sc, case.p, 3, rmax=rmax), case.want(1, radius)["within"], n, f"{which}, rmax {radius}")
        if which == "q":
            w = case.want(16, "0.05")
            assert (w["m"] > 16).sum() >= 50 and w["cut_tie"].sum() >= 10           # (the CPU file's counts, of this very run)
        # the views of tensors the call allocates
        tri, dist, st, nf, pts = sc.nearest_triangles_device(_dev_points(case.p, 3), 4, want_points=True)
        want = case.want(4)
        assert tri.dtype == nf.dtype == torch.int32 and dist.dtype == st.dtype == pts.dtype == torch.float32
        assert tri.shape == (n, 4) and st.shape == (n, 4, 2) and pts.shape == (n, 4, 3) and nf.shape == (n,)
        assert np.array_equal(_np(tri), want["triangle"]) and np.array_equal(_bits(dist), want["record"][..., 1])
        assert np.array_equal(_bits(st), want["record"][..., 2:]) and np.array_equal(_bits(pts), _bits(want["point"]))
        assert np.array_equal(_np(nf), want["nfound"])
        assert np.array_equal(_np(sc.within_radius_device(_dev_points(case.p, 4))), want["within"])


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles", "far", "one", "s"])
def test_k1_is_the_closest_point_query(which, request):
    case = request.getfixturevalue("s_scene")[1] if which == "s" else request.getfixturevalue(which)
    n = len(case.p)
    with _open(case, request) as sc:
        for radius, stride in itertools.product(("none", "0.05", "twice"), STRIDES):
            rmax = _dev(case.radii[radius])
            dp = _dev_points(case.p, stride)
            rec1 = torch.full((n, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
            pts1 = torch.full((n, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            sc.closest_point_device(dp, rmax=rmax, out=(rec1, pts1), want_points=True)
            rec, nf, pts = _query(sc, case.p, 1, stride, rmax=case.radii[radius])
            assert np.array_equal(rec[:n, 0], _np(rec1).view(np.uint32)), f"{which}, rmax {radius}, stride {stride}"
            assert np.array_equal(pts[:n, 0], _bits(pts1)), f"{which}, rmax {radius}, stride {stride}"
            assert np.array_equal(nf[:n], (_np(rec1)[:, 0] >= 0).astype(np.int32))
            assert np.array_equal(_within(sc, case.p, stride, rmax=case.radii[radius])[:n], (_np(rec1)[:, 0] >= 0).astype(np.uint8))


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles", "far"])
def test_every_walk_and_builder_gives_the_same_bytes(which, request):
    case = request.getfixturevalue(which)
    n = len(case.p)
    radius = "0.05" if which == "q" else "twice"
    with R.Scene.load(case.path, device=0) as sc:
        def run(what, stride=4):
            for k in (4, 16):
                for rad, count_all in ((radius, False), (radius, True), ("none", False)):
                    _check(_query(sc, case.p, k, stride, rmax=case.radii[rad], count_all=count_all), case.want(k, rad), n,
                           f"{which}, {what}, k {k}, rmax {rad}, count_all {count_all}", count_all=count_all)
            _check_within(_within(sc, case.p, stride, rmax=case.radii[radius]), case.want(1, radius)["within"], n, f"{which}, {what}")

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
        sc.tune("lds_stack", 1)
        run("binary, lds_stack 1")
        sc.tune("lds_stack", 16)
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


# 4 -------------------------------------------------------------------------------------------------
def test_far_tiny_walks_equal_brute_force_near_the_triangles(far):
    """4,096 points within a few edge lengths of triangles of a few ulps at 2^10: the computed closest point is
    rounded at the magnitude of the coordinates and can lie outside a triangle's box, so a box bound that is not
    deflated loses a list member. Every tree against the loop over all triangles, k = 8."""
    p = CP.near_far_points(far.T)
    n = len(p)
    small = np.full(n, 24 * CP.FAR_ULP, F32)

    def runs(sc):
        return (_query(sc, p, 8, 4), _query(sc, p, 8, 3, rmax=small, count_all=True), _within(sc, p, 4, rmax=np.full(n, 10 * CP.FAR_ULP, F32)))

    with R.Scene.load(far.path, device=0) as sc:
        sc.set_accel("brute_force")
        ref = runs(sc)
        tri = ref[0][0][:n, :, 0].view(np.int32)
        assert (tri >= 0).all() and (tri < CP.N_FAR).all() and len(np.unique(tri)) >= 100
        assert (ref[0][0][:n, :, 1].view(F32) <= 8 * CP.FAR_ULP).sum() >= 1000      # distances of the size of the rounding of c
        m = ref[1][1][:n]
        assert (m > 8).sum() >= 100 and ((m > 0) & (m < 8)).sum() >= 100             # lists cut and lists not full
        assert 1000 <= ref[2][:n].sum() <= n - 1000                             # about half the points answer
        # the brute-force rows against the closest-point query's (k = 1 is place 0 of k = 8)
        rec1 = torch.empty((n, 4), dtype=torch.int32, device=DEV)
        sc.closest_point_device(_dev_points(p, 3), out=rec1)
        assert np.array_equal(ref[0][0][:n, 0], _np(rec1).view(np.uint32))
        sc.set_accel("bvh")
        v = sc.export()["vertices"]
        for builder in ("sah", "lbvh", "cluster"):
            sc.set_builder(builder)
            sc.update_vertices(v, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                got = runs(sc)
                for a, b in zip(got[:2], ref[:2]):
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"{builder}, width {width}"
                assert np.array_equal(got[2], ref[2]), f"{builder}, width {width}: verdicts"


# 5 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "far"])
def test_radius_menu(which, request):
    case = request.getfixturevalue(which)
    n = len(case.p)
    dist = CP.closest(case.P)["distance"]
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
            stride = 3 if accel == "bvh" else 4
            for name, rmax in menu.items():
                what = f"{which}, {accel}, rmax {name}"
                want = NR.nearest(case.P, 4, rmax)
                for count_all in (False, True):
                    _check(_query(sc, case.p, 4, stride, rmax=rmax, count_all=count_all), want, n, what, count_all=count_all)
                got = _within(sc, case.p, stride, rmax=rmax)
                _check_within(got, want["within"], n, what)
                tri = sc.closest_point_device(_dev_points(case.p, stride), rmax=_dev(rmax))[0]
                assert np.array_equal(got[:n], (_np(tri) >= 0).astype(np.uint8)), what
                if name in ("half the distance", "zero", "negative", "nan"):
                    assert (want["m"][dist > 0] == 0).all(), name
                elif name == "+inf":
                    assert np.array_equal(want["record"], case.want(4)["record"])
                elif name == "the distance" and which == "q":
                    assert 10 <= want["within"].sum() <= (dist < np.inf).sum() - 10, name   # rmax * rmax on either side of dist2


# 6 -------------------------------------------------------------------------------------------------
def test_counts_and_sentinels(q):
    rmax = q.radii["0.05"]
    with R.Scene.load(q.path, device=0) as sc:
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            for n in (1, 63, 64, 65, 257):
                _check(_query(sc, q.p, 4, 3, rmax=rmax, n=n), q.want(4, "0.05"), n, f"{accel}, n {n}")
                _check_within(_within(sc, q.p, 3, rmax=rmax, n=n), q.want(1, "0.05")["within"], n, f"{accel}, n {n}")
                for c in (n - 1, n, n + 5, 0, -3):
                    live = min(max(c, 0), n)
                    cnt = torch.tensor([c], dtype=torch.int32, device=DEV)
                    what = f"{accel}, n {n}, count {c}"
                    _check(_query(sc, q.p, 4, 4, rmax=rmax, n=n, count=cnt, count_all=True), q.want(4, "0.05"), live, what, count_all=True)
                    _check(_query(sc, q.p, 16, 3, n=n, count=cnt, want_points=False), q.want(16), live, what, points=False)
                    _check_within(_within(sc, q.p, 4, rmax=rmax, n=n, count=cnt), q.want(1, "0.05")["within"], live, what)
        sc.set_accel("bvh")
        # rows a device count leaves unwritten in tensors the call allocates are the miss record and a count of 0
        cnt = torch.tensor([40], dtype=torch.int32, device=DEV)
        tri, dist, st, nf, pts = sc.nearest_triangles_device(_dev_points(q.p[:65], 3), 4, count=cnt, want_points=True)
        assert np.array_equal(_np(tri)[:40], q.want(4)["triangle"][:40]) and (_np(tri)[40:] == -1).all()
        assert np.isinf(_np(dist)[40:]).all() and (_np(st)[40:] == 0).all() and (_np(pts)[40:] == 0).all()
        assert np.array_equal(_np(nf)[:40], q.want(4)["nfound"][:40]) and (_np(nf)[40:] == 0).all()
        w = sc.within_radius_device(_dev_points(q.p[:65], 3), count=cnt)
        assert np.array_equal(_np(w)[:40], q.want(1)["within"][:40]) and (_np(w)[40:] == 0).all()
        # n == 0
        res = sc.nearest_triangles_device(torch.zeros((0, 3), dtype=torch.float32, device=DEV), 4)
        assert res[0].shape == (0, 4) and res[2].shape == (0, 4, 2) and res[3].shape == (0,)
        assert sc.within_radius_device(torch.zeros((0, 4), dtype=torch.float32, device=DEV)).shape == (0,)


# 7 -------------------------------------------------------------------------------------------------
def test_empty_and_degenerate_meshes(one, workdir):
    p = one.p
    n = len(p)

    def miss(k):
        return dict(record=np.tile(MISS, (n, k, 1)), point=np.zeros((n, k, 3), F32), nfound=np.zeros(n, np.int32), m=np.zeros(n, np.int32))

    nothing = np.zeros(n, np.uint8)
    deg = CP.degenerate_triangles()
    with R.Scene.load(CP.write_obj(workdir, "near_degenerate", deg), device=0) as sc:
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            for stride in STRIDES:
                _check(_query(sc, p, 4, stride, count_all=True), miss(4), n, f"degenerate, {accel}", count_all=True)
                _check_within(_within(sc, p, stride), nothing, n, f"degenerate, {accel}")
    with R.Scene.load(one.path, device=0) as sc:
        # one triangle, k = 16: one row, 15 miss rows
        want = one.want(16)
        hit = want["nfound"] == 1
        assert 240 <= hit.sum() <= n - 11 and (want["nfound"][~hit] == 0).all() and (want["record"][:, 1:] == MISS).all()
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            _check(_query(sc, p, 16, 3, count_all=True), want, n, f"one triangle, {accel}", count_all=True)
            _check_within(_within(sc, p, 3), want["within"], n, f"one triangle, {accel}")
        sc.set_accel("bvh")
        sc.set_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32))
        for accel in ("bvh", "brute_force"):
            sc.set_accel(accel)
            _check(_query(sc, p, 2, 4), miss(2), n, f"empty, {accel}")
            _check_within(_within(sc, p, 4), nothing, n, f"empty, {accel}")
        sc.set_accel("bvh")
        v = deg.reshape(-1, 3)
        sc.set_mesh(v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3), np.zeros(len(deg), np.uint32))
        _check(_query(sc, p, 4, 3), miss(4), n, "degenerate through set_mesh")
        v = one.T.reshape(-1, 3)
        sc.set_mesh(v, np.arange(3, dtype=np.uint32).reshape(1, 3), np.zeros(1, np.uint32))
        _check(_query(sc, p, 16, 3), want, n, "one triangle again")


def test_always_list_and_never_class_after_refit_and_set_mesh(s_scene, shingles):
    """Scene S holds a sliver (tested for every point, outside the tree) and a zero-area triangle (no candidate).
    The sliver appears in the lists of the three points next to it; after a refit on the device and after
    set_mesh from device tensors the answers are those of the restatement on the new triangles."""
    arr, before = s_scene
    p = before.p
    n = len(p)
    tri_idx = arr["triangles"].astype(np.int64)
    sliver = len(before.T) - 2
    assert not before.P["candidate"][0, -1] and before.P["candidate"][0, :-1].all()
    w4 = before.want(4)
    assert (w4["triangle"][-3:, 0] == sliver).all()                                # first there ...
    assert ((before.want(16)["triangle"] == sliver).any(axis=1)).sum() > 3         # ... and further down other lists
    assert not (before.want(16, "none")["triangle"] == len(before.T) - 1).any()    # the zero-area triangle: never
    new = S.deform(arr["vertices"], 0.03)
    after = Case(new[tri_idx], p)
    assert not np.array_equal(after.want(4)["record"], w4["record"])
    with S.create(arr, device=0) as sc:
        for width in (4, 2):
            sc.tune("bvh_width", width)
            for k in (4, 16):
                _check(_query(sc, p, k, 3, count_all=True), before.want(k), n, f"S, width {width}, k {k}", count_all=True)
            _check(_query(sc, p, 4, 3, rmax=before.radii["twice"]), before.want(4, "twice"), n, f"S, width {width}, twice")
            _check_within(_within(sc, p, 3, rmax=before.radii["0.05"]), before.want(1, "0.05")["within"], n, f"S, width {width}")
        sc.tune("bvh_width", 4)
        assert sc.update_vertices(torch.from_numpy(new).to(DEV)) == "refit"
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _check(_query(sc, p, 4, 4, count_all=True), after.want(4), n, f"S after the refit, width {width}", count_all=True)
            _check(_query(sc, p, 16, 4, rmax=after.radii["twice"]), after.want(16, "twice"), n, f"S after the refit, width {width}, twice")
            _check_within(_within(sc, p, 4, rmax=after.radii["0.05"]), after.want(1, "0.05")["within"], n, f"S after the refit, width {width}")
        # another mesh altogether, from device tensors: the shingles, then answers for the shingles' points
        v = torch.from_numpy(np.ascontiguousarray(shingles.T.reshape(-1, 3))).to(DEV)
        t = torch.arange(3 * len(shingles.T), dtype=torch.int32, device=DEV).reshape(-1, 3)
        m = torch.zeros(len(shingles.T), dtype=torch.int32, device=DEV)
        sc.set_mesh(v, t, m)
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _check(_query(sc, shingles.p, 8, 3, rmax=shingles.radii["twice"], count_all=True), shingles.want(8, "twice"), len(shingles.p),
                   f"after set_mesh_device, width {width}", count_all=True)
            _check_within(_within(sc, shingles.p, 3, rmax=shingles.radii["twice"]), shingles.want(1, "twice")["within"], len(shingles.p),
                          f"after set_mesh_device, width {width}")


# 8 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(q):
    """A query queued before update_vertices answers for the old vertices, one queued after it for the new; on a
    stream that is not the default."""
    st = torch.cuda.Stream(device=DEV)
    reps, n, k = 16, len(q.p), 4
    with R.Scene.load(q.path, device=0) as sc:
        e = sc.export()
        new = S.deform(e["vertices"], 0.03)
        moved = Case(new[e["triangles"].astype(np.int64)], q.p)
        old, now = q.want(k, "0.05"), moved.want(k, "0.05")
        assert (now["record"] != old["record"]).any(axis=(1, 2)).sum() >= 50
        with torch.cuda.stream(st):
            dp = _dev_points(q.p, 3)
            rm = _dev(q.radii["0.05"])
            tri, dist, sts, nf, pts = sc.nearest_triangles_device(dp.repeat(reps, 1), k, rmax=rm.repeat(reps), want_points=True)   # (the current stream: st)
            w = sc.within_radius_device(dp.repeat(reps, 1), rmax=rm.repeat(reps))
        assert sc.update_vertices(new) == "refit"
        with torch.cuda.stream(st):
            tri2, dist2, sts2, nf2, pts2 = sc.nearest_triangles_device(dp, k, rmax=rm, want_points=True, stream=st)
            w2 = sc.within_radius_device(dp, rmax=rm, stream=st)
        st.synchronize()
        assert np.array_equal(_np(tri).reshape(reps, n, k), np.tile(old["triangle"], (reps, 1, 1)))
        assert np.array_equal(_bits(dist).reshape(reps, n, k), np.tile(old["record"][..., 1], (reps, 1, 1)))
        assert np.array_equal(_bits(sts).reshape(reps, n, k, 2), np.tile(old["record"][..., 2:], (reps, 1, 1, 1)))
        assert np.array_equal(_bits(pts).reshape(reps, n, k, 3), np.tile(_bits(old["point"]), (reps, 1, 1, 1)))
        assert np.array_equal(_np(nf).reshape(reps, n), np.tile(old["nfound"], (reps, 1)))
        assert np.array_equal(_np(w).reshape(reps, n), np.tile(old["within"], (reps, 1)))
        assert np.array_equal(_np(tri2), now["triangle"]) and np.array_equal(_bits(dist2), now["record"][..., 1])
        assert np.array_equal(_bits(sts2), now["record"][..., 2:]) and np.array_equal(_bits(pts2), _bits(now["point"]))
        assert np.array_equal(_np(nf2), now["nfound"]) and np.array_equal(_np(w2), now["within"])


# 9 -------------------------------------------------------------------------------------------------
def test_the_walk_culls(q):
    """With RT_PROFILE_WORK the point-triangle evaluations per point on scene Q, for 256 points uniform in the
    scene's box with rmax = 0.05, of the k = 16 list and of the verdict: strictly below the triangle count (the
    loop over all triangles evaluates every one) and at most 1.25 x what profiles/nearest_probe.json records for
    each builder and width (the count is deterministic per tree; the margin covers later changes of tree shape
    only). The verdict evaluates no more than the k = 1 list: it is that walk up to the first candidate."""
    with open(os.path.join(ROOT, "profiles", "nearest_probe.json")) as f:
        measured = json.load(f)["scene_q_work"]
    p = CP.in_box_points(q.T)
    n, nt = len(p), len(q.T)
    assert nt == 1640 and measured["triangles"] == nt and measured["points"] == n and measured["rmax"] == 0.05
    rmax = np.full(n, 0.05, F32)
    P = CP.pairs(p, q.T)
    want16, want1 = NR.nearest(P, 16, rmax), NR.nearest(P, 1, rmax)
    assert (want16["m"] > 0).sum() >= 20
    with R.Scene.load(q.path, device=0) as sc:
        v = sc.export()["vertices"]
        sc.set_profiling(True, count_work=True)
        for builder in ("sah", "lbvh", "cluster"):
            sc.set_builder(builder)
            sc.update_vertices(v, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                what = f"{builder}, width {width}"
                pinned = measured[builder][f"width{width}"]
                sc.reset_stats()
                _check(_query(sc, p, 16, 3, rmax=rmax), want16, n, what)
                t16, v16 = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                sc.reset_stats()
                _check(_query(sc, p, 1, 3, rmax=rmax), want1, n, what)
                t1, _ = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                sc.reset_stats()
                _check_within(_within(sc, p, 3, rmax=rmax), want1["within"], n, what)
                tw, vw = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                print(f"{what}: k = 16 {t16 / n:.3f} evaluations, {v16 / n:.3f} node visits per point (recorded "
                      f"{pinned['k16_evaluations_per_point']}); k = 1 {t1 / n:.3f}; verdict {tw / n:.3f}, {vw / n:.3f} (recorded "
                      f"{pinned['within_evaluations_per_point']})")
                assert 0 < t16 / n < nt and 0 < tw / n < nt
                assert t16 / n <= 1.25 * pinned["k16_evaluations_per_point"], what
                assert tw / n <= 1.25 * pinned["within_evaluations_per_point"], what
                assert tw <= t1, what
        sc.set_profiling(False)


# 10 ------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(q):
    """Each RT_E_ARG case alone on a scene with a device; nothing is written."""
    L = _capi.lib()
    k = 4
    dp = _dev_points(q.p[:8], 4)
    rec = torch.full((16, k, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    nf = torch.full((16,), NF_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((16, k, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    wi = torch.full((16,), W_SENTINEL, dtype=torch.uint8, device=DEV)
    rb = torch.ones(16, dtype=torch.float32, device=DEV)
    cnt = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with R.Scene.load(q.path, device=0) as sc:
        good = dict(p=vp(dp), stride=4, n=8, count=vp(cnt), rmax=vp(rb), flags=0, k=k, out=vp(rec), nf=vp(nf), out2=vp(pts), w=vp(wi))

        def near(**kw):
            a = dict(good, **kw)
            return L.rt_nearest_triangles_device(sc.handle, a["p"], a["stride"], a["n"], a["count"], a["rmax"], a["flags"], a["k"],
                                                 a["out"], a["nf"], a["out2"], None)

        def within(**kw):
            a = dict(good, **kw)
            return L.rt_within_radius_device(sc.handle, a["p"], a["stride"], a["n"], a["count"], a["rmax"], a["flags"], a["w"], None)

        shared = [dict(n=-1), dict(stride=5), dict(stride=0), dict(p=None), dict(p=vp(dp, 4), n=7), dict(stride=3, p=vp(dp, 2)),
                  dict(count=vp(cnt, 2)), dict(rmax=vp(rb, 1)), dict(flags=1 << 31), dict(flags=_capi.RANGE_TO_DEST),
                  dict(flags=_capi.OCCLUDE_ANY_OPAQUE), dict(flags=_capi.MULTI_COUNT_ALL)]
        for kw in shared + [dict(out=None), dict(out=vp(rec, 8)), dict(out=vp(rec, 4)), dict(nf=vp(nf, 2)), dict(out2=vp(pts, 2)),
                            dict(k=0), dict(k=-1), dict(k=_capi.MULTI_HIT_MAX + 1), dict(flags=_capi.NEAR_COUNT_ALL, nf=None),
                            dict(flags=_capi.NEAR_COUNT_ALL | _capi.RANGE_TO_DEST), dict(n=(1 << 31) // 16, k=16)]:
            assert near(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        for kw in shared + [dict(w=None), dict(flags=_capi.NEAR_COUNT_ALL), dict(flags=1)]:
            assert within(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        assert near(n=0, p=None, out=None, nf=None, out2=None) == _capi.RT_OK     # n == 0: nothing to do
        assert within(n=0, p=None, w=None) == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(rec) == REC_SENTINEL).all() and (_np(nf) == NF_SENTINEL).all() and (_bits(pts) == NAN_SENTINEL).all()
        assert (_np(wi) == W_SENTINEL).all()                                      # nothing was written
        assert near() == _capi.RT_OK and within() == _capi.RT_OK
        assert near(nf=None, out2=None) == _capi.RT_OK                            # both optional without the flag
        torch.cuda.synchronize()
        assert (_np(rec)[:8, :, 0] != REC_SENTINEL).all() and (_np(rec)[8:] == REC_SENTINEL).all()
        assert (_np(nf)[:8] != NF_SENTINEL).all() and (_np(nf)[8:] == NF_SENTINEL).all()
        assert (_bits(pts)[:8] != NAN_SENTINEL).all() and (_bits(pts)[8:] == NAN_SENTINEL).all()
        assert (_np(wi)[:8] <= 1).all() and (_np(wi)[8:] == W_SENTINEL).all()
        for kw in (dict(rmax=torch.ones(4, dtype=torch.float32, device=DEV)), dict(out=(rec[:4], nf)), dict(out=(rec, nf[:4])),
                   dict(out=rec), dict(out=(rec, nf), want_points=True), dict(out=(rec, nf, pts[:, :2]), want_points=True),
                   dict(out=(torch.zeros((16, k + 1, 4), dtype=torch.int32, device=DEV), nf))):
            with pytest.raises(ValueError):
                sc.nearest_triangles_device(dp, k, **kw)
        for kw in (dict(rmax=torch.ones(4, dtype=torch.float32, device=DEV)), dict(out=wi[:4]), dict(out=nf)):
            with pytest.raises(ValueError):
                sc.within_radius_device(dp, **kw)
