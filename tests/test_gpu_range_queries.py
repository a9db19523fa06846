"""Ranged device queries (rt_closest_hit_range_device, rt_occluded_range_device: k_bvh_range_rays,
k_range_rays): hit records {triangle, distance, s, t} and verdict bytes for rays with a per-ray distance range
[tmin, tmax), rays and results in torch CUDA tensors.

The expectation is tests/_range_ref.py, the numpy restatement that tests/test_range_ref.py pins to the oracle
on the CPU (and whose counts say that no case below passes empty). Equality is of bytes throughout: there is no
tolerance. Scenes Q and Qo with ray set R200 (tests/_query_scenes.py), shingles / shingles_tr with the generic
rays and the long and short classes (tests/_edge_rays.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _edge_rays as E
import _query_scenes as QS
import _range_ref as RR
import _refit_scenes as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
CAP = 264                      # output rows allocated (more than any n of the sentinel checks)
REC_SENTINEL = -7
NAN_SENTINEL = 0x7FC0DEAD      # a NaN bit pattern no kernel computes
BLK_SENTINEL = 0xEE
STRIDES = (3, 4)
INF = F32(np.inf)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _dev_rays(o, d, stride):
    """The rays as CUDA tensors in either layout; the padded layout's w holds values that must not matter."""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    if stride == 4:
        o = np.concatenate([o, np.full((len(o), 1), 123.0, F32)], axis=1)
        d = np.concatenate([d, np.full((len(d), 1), np.nan, F32)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(o)).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


class Case:
    """One scene file, its rays, and every ray x triangle pair by the helper (computed once, never changed)."""

    def __init__(self, path, o, d):
        self.path, self.o, self.d = path, o, d
        self.T, self.transparent = RR.scene_triangles(O.OracleScene(path))
        self.P = RR.pairs(o, d, self.T)
        for a in self.P.values():
            a.setflags(write=False)
        self.len = RR.ray_length(o, d)
        self.d1, self.d2, self.d3 = (RR.nth_distance(self.P, k) for k in range(3))

    def bounds(self, **kw):
        return RR.bounds(self.o, self.d, **kw)

    def closest(self, **kw):
        return RR.closest(self.P, *self.bounds(**kw))

    def occluded(self, any_opaque, **kw):
        return RR.occluded(self.P, *self.bounds(**kw), self.transparent, any_opaque)

    def menu(self):
        """name -> dict(tmin, tmax, to_dest): the range cases (per-ray float32 arrays or None)."""
        up = lambda a: np.nextafter(a, INF).astype(F32)
        return {
            "half-line": dict(),
            "to dest": dict(to_dest=True),
            "twice the length": dict(tmax=(F32(2) * self.len).astype(F32)),
            "tmax = closest": dict(tmax=self.d1),
            "tmax just above closest": dict(tmax=up(self.d1)),
            "tmin = closest": dict(tmin=self.d1),
            "tmin just above closest": dict(tmin=up(self.d1)),
            "second to third": dict(tmin=self.d2, tmax=self.d3),
        }


@pytest.fixture(scope="module")
def q(workdir, gpu_available):
    return Case(scenes.write_sphere_grid(QS.SPEC_Q, workdir, "range_q"), *QS.r200())


@pytest.fixture(scope="module")
def qo(workdir, gpu_available):
    return Case(scenes.write_sphere_grid(QS.SPEC_QO, workdir, "range_qo"), *QS.r200())


@pytest.fixture(scope="module")
def shingles(workdir, gpu_available):
    return Case(E.write_scene(workdir, "range_shingles"), *E.generic())


@pytest.fixture(scope="module")
def shingles_tr(workdir, gpu_available):
    return Case(E.write_scene(workdir, "range_shingles_tr", transparent=True), *E.generic())


@pytest.fixture(scope="module")
def shingles_big(workdir, gpu_available):
    o, d = E.generic()
    return Case(E.write_scene(workdir, "range_shingles_big", transparent=True, scale=E.BIG), o * F32(E.BIG), d * F32(E.BIG))


def _closest(sc, o, d, stride, tmin=None, tmax=None, to_dest=False, count=None, n=None):
    """One closest-record query into sentinel-filled outputs: (records [CAP, 4] uint32, point bits [CAP, 3])."""
    n = len(o) if n is None else n
    cap = max(CAP, len(o) + 8)
    do, dd = _dev_rays(o[:n], d[:n], stride)
    rec = torch.full((cap, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((cap, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    res = sc.closest_hit_device(do, dd, tmin=_dev(tmin), tmax=_dev(tmax), to_dest=to_dest, count=count, out=(rec, pts),
                                want_points=True)
    assert len(res) == 4 and res[0].shape == (n,) and res[1].shape == (n,) and res[2].shape == (n, 2) and res[3].shape == (n, 3)
    assert res[0].data_ptr() == rec.data_ptr() and res[0].dtype == torch.int32 and res[1].dtype == torch.float32
    return _np(rec).view(np.uint32), _bits(pts)


def _blocked(sc, o, d, stride, any_opaque, tmin=None, tmax=None, to_dest=False, count=None, n=None):
    n = len(o) if n is None else n
    do, dd = _dev_rays(o[:n], d[:n], stride)
    blk = torch.full((max(CAP, len(o) + 8),), BLK_SENTINEL, dtype=torch.uint8, device=DEV)
    res = sc.occluded_range_device(do, dd, tmin=_dev(tmin), tmax=_dev(tmax), to_dest=to_dest, any_opaque=any_opaque, count=count, out=blk)
    assert res.shape == (n,) and res.data_ptr() == blk.data_ptr()
    return _np(blk)


def _check_records(got, want, live, what=""):
    rec, pts = got
    bad = np.flatnonzero((rec[:live] != want["record"][:live]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} records differ, first rays {bad[:5]}: {rec[bad[:5]]} for {want['record'][bad[:5]]}"
    assert np.array_equal(pts[:live], _bits(want["point"][:live])), f"{what}: points differ"
    assert (rec[live:].view(np.int32) == REC_SENTINEL).all() and (pts[live:] == NAN_SENTINEL).all(), f"{what}: rows past {live} written"


def _check_blocked(got, want, live, what=""):
    assert np.array_equal(got[:live], want[:live]), f"{what}: {np.flatnonzero(got[:live] != want[:live])[:8]}"
    assert (got[live:] == BLK_SENTINEL).all(), f"{what}: rows past {live} written"


def _check_all(case, sc, kw, what, strides=STRIDES):
    """The closest record and both occlusion rules of one range case against the helper; the helper's answers."""
    want = case.closest(**kw)
    rules = {ao: case.occluded(ao, **kw) for ao in (False, True)}
    n = len(case.o)
    for stride in strides:
        _check_records(_closest(sc, case.o, case.d, stride, **kw), want, n, f"{what}, stride {stride}")
        for ao in (False, True):
            _check_blocked(_blocked(sc, case.o, case.d, stride, ao, **kw), rules[ao], n, f"{what}, any_opaque {ao}, stride {stride}")
    return want, rules


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "qo", "shingles", "shingles_tr"])
def test_null_bounds_are_the_half_line_entries(which, request):
    case = request.getfixturevalue(which)
    n = len(case.o)
    want = case.closest()
    miss = want["triangle"] < 0
    assert 20 <= miss.sum() <= n - 100
    assert (want["record"][miss] == np.array([0xFFFFFFFF, RR.INF_BITS, 0, 0], np.uint32)).all()
    with R.Scene.load(case.path, device=0) as sc:
        for stride in STRIDES:
            do, dd = _dev_rays(case.o, case.d, stride)
            idx, pts = sc.intersect_mesh_device(do, dd)
            blk = sc.occluded_device(do, dd)
            rec, rpts = _closest(sc, case.o, case.d, stride)
            assert np.array_equal(rec[:n, 0].view(np.int32), _np(idx)) and np.array_equal(rpts[:n], _bits(pts))
            _check_records((rec, rpts), want, n, f"{which}, stride {stride}")
            _check_blocked(_blocked(sc, case.o, case.d, stride, False), _np(blk), n, "default rule against rt_occluded_device")
            _check_blocked(_blocked(sc, case.o, case.d, stride, True), case.occluded(True), n, "any opaque")
            # without points, and the views of a record tensor the call allocates
            tri, dist, st = sc.closest_hit_device(do, dd)
            assert tri.dtype == torch.int32 and dist.dtype == st.dtype == torch.float32 and st.shape == (n, 2)
            assert np.array_equal(_np(tri), want["triangle"]) and np.array_equal(_bits(dist), want["record"][:, 1])
            assert np.array_equal(_bits(st), want["record"][:, 2:])


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "qo", "shingles", "shingles_tr"])
def test_range_cases(which, request):
    case = request.getfixturevalue(which)
    half = case.closest()["triangle"]
    hit = half >= 0
    differ = {}
    with R.Scene.load(case.path, device=0) as sc:
        for name, kw in case.menu().items():
            want, rules = _check_all(case, sc, kw, f"{which}, {name}")
            differ[name] = int((rules[False] != rules[True]).sum())
            tri = want["triangle"]
            if name == "tmax = closest":
                assert (tri < 0).all()                                   # strict '<': the closest itself is out
            if name in ("tmax just above closest", "tmin = closest"):
                assert np.array_equal(tri, half)
            if name == "tmin just above closest":
                assert (tri[hit] != half[hit]).all() and (tri >= 0).sum() >= 80 and (tri[hit] < 0).sum() >= (0 if which.startswith("s") else 70)
            if name == "second to third" and which.startswith("shingles"):
                assert (tri[hit] >= 0).all() and (want["distance"][hit] == case.d2[hit]).all()
            if name in ("to dest", "twice the length"):
                assert 90 <= (tri >= 0).sum() <= hit.sum()
    if which in ("q", "shingles_tr"):      # the two rules are told apart (tests/test_range_ref.py has the counts)
        assert differ["half-line"] >= 27 and differ["to dest"] >= 1 and differ["twice the length"] >= 27
    else:
        assert not any(differ.values())


# 3 -------------------------------------------------------------------------------------------------
def test_peeling_walks_every_accepted_triangle_in_order(shingles):
    """tmin = nextafter(previous distance) until every ray misses: per ray the helper's sorted accepted list."""
    case = shingles
    n = len(case.o)
    want = [RR.sorted_hits(case.P, i) for i in range(n)]
    assert max(len(w) for w in want) == 36
    for w in want:
        assert all(a[0] < b[0] for a, b in zip(w, w[1:]))       # no two at one distance: nextafter skips none
    got = [[] for _ in range(n)]
    with R.Scene.load(case.path, device=0) as sc:
        do, dd = _dev_rays(case.o, case.d, 3)
        tmin = None
        for launch in range(38):
            tri, dist, _ = sc.closest_hit_device(do, dd, tmin=tmin)
            tri_h, dist_h = _np(tri), _np(dist)
            if (tri_h < 0).all():
                break
            for i in np.flatnonzero(tri_h >= 0):
                got[i].append((float(dist_h[i]), int(tri_h[i])))
            tmin = torch.nextafter(dist, torch.full_like(dist, float("inf")))     # (+inf stays +inf: an empty range)
        assert launch == 36                                     # 36 layers, then the launch in which all miss
    assert got == want


# 4 -------------------------------------------------------------------------------------------------
def test_empty_ranges_report_misses(q):
    n = len(q.o)
    nan = F32(np.nan)
    kinds = [dict(tmin=nan), dict(tmax=nan), dict(tmax=F32(0)), dict(tmax=F32(-0.0)), dict(tmax=F32(-1)), dict(tmin=F32(5), tmax=F32(1)),
             dict(tmin=INF), dict(tmin=F32(1), tmax=F32(1)), dict(tmin=nan, tmax=nan), dict(tmax=-INF)]
    assert (q.closest()["triangle"] >= 0).sum() == 161
    with R.Scene.load(q.path, device=0) as sc:
        for kind in kinds:
            kw = {k: np.full(n, v, F32) for k, v in kind.items()}
            want, rules = _check_all(q, sc, kw, str(kind))
            assert (want["triangle"] < 0).all() and not rules[False].any() and not rules[True].any()
        # ... also next to rays that walk, in one wave: every third ray keeps its half-line range
        tmin, tmax = np.zeros(n, F32), np.full(n, np.inf, F32)
        for i in range(n):
            if i % 3:
                kind = kinds[i % len(kinds)]
                tmin[i], tmax[i] = kind.get("tmin", F32(0)), kind.get("tmax", INF)
        want, _ = _check_all(q, sc, dict(tmin=tmin, tmax=tmax), "empty ranges among live ones")
        assert (want["triangle"][np.arange(n) % 3 != 0] < 0).all() and (want["triangle"][::3] >= 0).sum() >= 40


# 5 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles_tr"])
def test_mixed_menu_in_one_wave(which, request):
    """Ray i takes menu entry i mod 8, as explicit per-ray bounds: one wave holds divergent ranges."""
    case = request.getfixturevalue(which)
    n = len(case.o)
    tmin, tmax = np.zeros(n, F32), np.full(n, np.inf, F32)
    for k, kw in enumerate(case.menu().values()):
        rows = np.arange(n) % 8 == k
        if kw.get("to_dest"):
            tmax[rows] = case.len[rows]
        if kw.get("tmin") is not None:
            tmin[rows] = kw["tmin"][rows]
        if kw.get("tmax") is not None:
            tmax[rows] = kw["tmax"][rows]
    with R.Scene.load(case.path, device=0) as sc:
        want, rules = _check_all(case, sc, dict(tmin=tmin, tmax=tmax), which + ", mixed menu")
    assert 60 <= (want["triangle"] >= 0).sum() <= n - 40 and (rules[False] != rules[True]).any()


# 6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_prefixes_by_n_and_by_device_count(q, stride):
    two = (F32(2) * q.len).astype(F32)
    want = q.closest(tmax=two)
    rules = {ao: q.occluded(ao, tmax=two) for ao in (False, True)}
    assert [int((want["triangle"][:n] >= 0).sum()) for n in QS.PREFIXES] == [1, 63, 64, 65, 123, 157]
    with R.Scene.load(q.path, device=0) as sc:
        for n in QS.PREFIXES:
            _check_records(_closest(sc, q.o, q.d, stride, tmax=two[:n], n=n), want, n, f"n {n}")
            for ao in (False, True):
                _check_blocked(_blocked(sc, q.o, q.d, stride, ao, tmax=two[:n], n=n), rules[ao], n, f"n {n}")
        for count, live in [(c, c) for c in QS.PREFIXES] + [(0, 0), (1000, 200), (-5, 0)]:
            cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
            _check_records(_closest(sc, q.o, q.d, stride, tmax=two, count=cnt), want, live, f"count {count}")
            for ao in (False, True):
                _check_blocked(_blocked(sc, q.o, q.d, stride, ao, tmax=two, count=cnt), rules[ao], live, f"count {count}")
            # outputs the call allocates: rows past the live count hold the miss record / 0
            do, dd = _dev_rays(q.o, q.d, stride)
            tri, dist, st, pts = sc.closest_hit_device(do, dd, tmax=_dev(two), count=cnt, want_points=True)
            blk = sc.occluded_range_device(do, dd, tmax=_dev(two), count=cnt)
            assert np.array_equal(_np(tri)[:live], want["triangle"][:live]) and (_np(tri)[live:] == -1).all()
            assert (_bits(dist)[live:] == RR.INF_BITS).all() and (_bits(st)[live:] == 0).all() and (_bits(pts)[live:] == 0).all()
            assert np.array_equal(_np(blk)[:live], rules[False][:live]) and (_np(blk)[live:] == 0).all()


# 7 -------------------------------------------------------------------------------------------------
def _menu_subset(case):
    m = case.menu()
    return {k: m[k] for k in ("half-line", "to dest", "tmin just above closest", "second to third")}


@pytest.mark.parametrize("which", ["q", "shingles_tr"])
def test_every_traversal_gives_the_same_bytes(which, request):
    case = request.getfixturevalue(which)
    with R.Scene.load(case.path, device=0) as sc:
        assert sc.accel() == "bvh"

        def run(what):
            for name, kw in _menu_subset(case).items():
                _check_all(case, sc, kw, f"{which}, {what}, {name}", strides=(3,))

        run("four-wide")
        sc.set_profiling(True, count_work=True)                 # the counting instantiations
        sc.reset_stats()
        run("four-wide, counting")
        assert sc.work_stats(_capi.KERNEL_CLOSEST_HIT)[1] > 0 and sc.work_stats(_capi.KERNEL_SHADOW)[1] > 0
        sc.tune("bvh_width", 2)
        run("binary, counting")
        sc.set_profiling(False)
        run("binary")
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        run("brute force")
        sc.set_accel("bvh")
        v = sc.export()["vertices"]
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(v, "rebuild") == "rebuilt_" + builder
            run(builder)


def test_scaled_scene_takes_the_binary_walk(shingles_big):
    """Shingles times 2^21 (scene_m1 >= 1e6: the binary tree whatever bvh_width says), one material transparent."""
    case = shingles_big
    assert (case.closest()["triangle"] >= 0).sum() >= 150
    with R.Scene.load(case.path, device=0) as sc:
        assert np.abs(sc.export()["vertices"]).sum(axis=1).max() >= 1e6
        for name, kw in case.menu().items():
            _check_all(case, sc, kw, "scaled, " + name, strides=(4,))


# 8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ["B", "C"])
def test_long_and_short_rays(shingles_tr, letter):
    """Class B (dot(dir, dir) overflows: the walks' distance cull is off) and C (short) with finite bounds from
    the helper: up to the second distance, the second-to-third window, the segment."""
    o, d, where = E.class_rays(letter)
    case = Case(shingles_tr.path, o, d)
    hit = case.d1 < INF
    assert hit.sum() >= (3 if letter == "B" else 2) * 150
    if letter == "B":
        with np.errstate(over="ignore"):
            e = d - o
            assert np.isinf((e * e).sum(axis=1).astype(F32)).all()
    menu = {"below the second": dict(tmax=case.d2), "second to third": dict(tmin=case.d2, tmax=case.d3), "to dest": dict(to_dest=True),
            "half-line": dict()}
    with R.Scene.load(case.path, device=0) as sc:
        for width in (4, 2):
            sc.tune("bvh_width", width)
            for name, kw in menu.items():
                want, _ = _check_all(case, sc, kw, f"class {letter}, width {width}, {name}", strides=(3,))
                if name == "below the second":
                    assert np.array_equal(want["triangle"] >= 0, hit)
                if name == "second to third":
                    assert (want["triangle"] >= 0).sum() >= hit.sum() - 20


# 9 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(q, workdir):
    """A ranged query queued before update_vertices answers for the old vertices, one queued after for the new."""
    st = torch.cuda.Stream(device=DEV)
    two = (F32(2) * q.len).astype(F32)
    old = q.closest(tmax=two)
    old_blk = q.occluded(True, tmax=two)
    reps = 16
    with R.Scene.load(q.path, device=0) as sc:
        e = sc.export()
        arr = dict(vertices=e["vertices"], triangles=e["triangles"], tri_mat=e["tri_mat"], materials=e["materials"],
                   mtl=q.path[:-4] + ".mtl")
        new = S.deform(e["vertices"], 0.03)
        moved = Case.__new__(Case)
        moved.o, moved.d = q.o, q.d
        moved.T = np.ascontiguousarray(new[e["triangles"].astype(np.int64)], F32)
        moved.transparent = q.transparent
        moved.P = RR.pairs(q.o, q.d, moved.T)
        new_want = moved.closest(tmax=two)
        assert not np.array_equal(new_want["record"], old["record"])
        with torch.cuda.stream(st):
            do, dd = _dev_rays(q.o, q.d, 3)
            bo, bd, bt = do.repeat(reps, 1), dd.repeat(reps, 1), _dev(two).repeat(reps)
            tri, dist, sts, pts = sc.closest_hit_device(bo, bd, tmax=bt, want_points=True)
            blk = sc.occluded_range_device(bo, bd, tmax=bt, any_opaque=True, stream=st)
        assert sc.update_vertices(new) == "refit"
        with torch.cuda.stream(st):
            tri2, dist2, sts2, pts2 = sc.closest_hit_device(do, dd, tmax=_dev(two), want_points=True)
            blk2 = sc.occluded_range_device(do, dd, tmax=_dev(two), any_opaque=True)
        st.synchronize()
        assert np.array_equal(_np(tri).reshape(reps, 200), np.tile(old["triangle"], (reps, 1)))
        assert np.array_equal(_bits(dist).reshape(reps, 200), np.tile(old["record"][:, 1], (reps, 1)))
        assert np.array_equal(_bits(sts).reshape(reps, 200, 2), np.tile(old["record"][:, 2:], (reps, 1, 1)))
        assert np.array_equal(_bits(pts).reshape(reps, 200, 3), np.tile(_bits(old["point"]), (reps, 1, 1)))
        assert np.array_equal(_np(blk).reshape(reps, 200), np.tile(old_blk, (reps, 1)))
        assert np.array_equal(_np(tri2), new_want["triangle"]) and np.array_equal(_bits(dist2), new_want["record"][:, 1])
        assert np.array_equal(_bits(sts2), new_want["record"][:, 2:]) and np.array_equal(_bits(pts2), _bits(new_want["point"]))
        assert np.array_equal(_np(blk2), moved.occluded(True, tmax=two))


# 10 ------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(q):
    """Each RT_E_ARG case alone on a scene with a device (tests/test_range_queries_capi.py has the table for the
    cases before a device); nothing is enqueued."""
    L = _capi.lib()
    do, dd = _dev_rays(q.o[:8], q.d[:8], 4)
    rec = torch.full((CAP, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((CAP, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    blk = torch.full((CAP,), BLK_SENTINEL, dtype=torch.uint8, device=DEV)
    tb = torch.ones(CAP, dtype=torch.float32, device=DEV)
    cnt = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with R.Scene.load(q.path, device=0) as sc:
        h = sc.handle
        good = dict(o=vp(do), d=vp(dd), stride=4, n=8, count=vp(cnt), tmin=vp(tb), tmax=vp(tb, 64), flags=_capi.RANGE_TO_DEST,
                    out=vp(rec), out2=vp(pts))

        def closest(**kw):
            a = dict(good, **kw)
            return L.rt_closest_hit_range_device(h, a["o"], a["d"], a["stride"], a["n"], a["count"], a["tmin"], a["tmax"], a["flags"],
                                                 a["out"], a["out2"], None)

        def occl(**kw):
            a = dict(dict(good, out=vp(blk)), **kw)
            return L.rt_occluded_range_device(h, a["o"], a["d"], a["stride"], a["n"], a["count"], a["tmin"], a["tmax"], a["flags"],
                                              a["out"], None)

        common = [dict(n=-1), dict(stride=5), dict(d=None), dict(o=vp(do, 4), n=7), dict(out=None), dict(count=vp(cnt, 2)),
                  dict(tmin=vp(tb, 1)), dict(tmax=vp(tb, 2)), dict(flags=1 << 2), dict(flags=(1 << 31) | 1)]
        for kw in common:
            assert closest(**kw) == _capi.RT_E_ARG, kw
            assert occl(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        for kw in (dict(out=vp(rec, 8)), dict(out=vp(rec, 4)), dict(out2=vp(pts, 2)), dict(flags=_capi.OCCLUDE_ANY_OPAQUE),
                   dict(flags=_capi.OCCLUDE_ANY_OPAQUE | _capi.RANGE_TO_DEST)):
            assert closest(**kw) == _capi.RT_E_ARG, kw
        assert closest(n=0, o=None, d=None, out=None, out2=None) == _capi.RT_OK          # n == 0: nothing to do
        assert occl(n=0, o=None, d=None, out=None) == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(rec) == REC_SENTINEL).all() and (_np(blk) == BLK_SENTINEL).all()       # nothing was enqueued
        assert (_bits(pts) == NAN_SENTINEL).all()
        # the Python forms
        with pytest.raises(ValueError):
            sc.closest_hit_device(do, dd, tmin=tb.cpu())
        with pytest.raises(ValueError):
            sc.closest_hit_device(do, dd, tmax=tb[:4])
        with pytest.raises(ValueError):
            sc.occluded_range_device(do, dd, tmin=tb.double())
        with pytest.raises(ValueError):
            sc.closest_hit_device(do, dd, out=rec[:4])
        with pytest.raises(ValueError):
            sc.closest_hit_device(do, dd, out=rec, want_points=True)
        with pytest.raises(ValueError):
            sc.occluded_range_device(do, dd, count=torch.zeros(1, dtype=torch.int32))
        e_tri, e_dist, e_st = sc.closest_hit_device(do[:0], dd[:0])
        assert e_tri.shape == (0,) and e_dist.shape == (0,) and e_st.shape == (0, 2)
