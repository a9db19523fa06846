"""The multi-hit device query (rt_multi_hit_range_device: k_bvh_multi_rays, k_multi_rays): per ray the first k
in-range accepted triangles in ascending (distance, index) order from one walk, and their number.

The expectation is tests/_multi_hit_ref.py, built from tests/_range_ref.py (pinned to the oracle on the CPU by
tests/test_range_ref.py; tests/test_multi_hit_ref.py says what the lists look like). Equality is of bytes
throughout: there is no tolerance. Scenes as tests/test_gpu_range_queries.py (Q and Qo with ray set R200, shingles
/ shingles_tr / the scaled shingles with the generic rays and the long and short classes), plus doubled shingles,
where every distance comes three times. Outputs are sentinel-filled and longer than n x k; every check also says
that the rows past the live rays kept the sentinel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _edge_rays as E
import _multi_hit_ref as MH
import _query_scenes as QS
import _range_ref as RR
import _refit_scenes as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
CAP = 264                      # output rays allocated (more than any n of the sentinel checks)
REC_SENTINEL = -7
NH_SENTINEL = -9
STRIDES = (3, 4)
INF = F32(np.inf)
KMAX = _capi.MULTI_HIT_MAX


def _np(t):
    return t.cpu().numpy()


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

    def __init__(self, path, o, d, T=None, transparent=None):
        self.path, self.o, self.d = path, o, d
        if T is None:
            T, transparent = RR.scene_triangles(O.OracleScene(path))
        self.T, self.transparent = T, transparent
        self.P = RR.pairs(o, d, self.T)
        for a in self.P.values():
            a.setflags(write=False)
        self.len = RR.ray_length(o, d)
        self.d1, self.d2, self.d3 = (RR.nth_distance(self.P, k) for k in range(3))
        self._memo = {}

    def bounds(self, **kw):
        return RR.bounds(self.o, self.d, **kw)

    def first_k(self, k, name=None, **kw):
        """(records, nhits, totals) of a range case; memoised under `name` (the expectation is shared, not rebuilt)."""
        key = (name, k)
        if name is None or key not in self._memo:
            b = self.bounds(**kw)
            res = MH.first_k(self.P, *b, k) + (MH.totals(self.P, *b),)
            if name is None:
                return res
            self._memo[key] = res
        return self._memo[key]

    def closest(self, **kw):
        return RR.closest(self.P, *self.bounds(**kw))

    def menu(self):
        """name -> dict(tmin, tmax, to_dest): the range cases of tests/test_gpu_range_queries.py."""
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

    def short_menu(self):
        m = self.menu()
        return {"half-line": m["half-line"], "to dest": m["to dest"], "tmin = second": dict(tmin=self.d2),
                "second to third": m["second to third"]}


@pytest.fixture(scope="module")
def q(workdir, gpu_available):
    return Case(scenes.write_sphere_grid(QS.SPEC_Q, workdir, "multi_q"), *QS.r200())


@pytest.fixture(scope="module")
def qo(workdir, gpu_available):
    return Case(scenes.write_sphere_grid(QS.SPEC_QO, workdir, "multi_qo"), *QS.r200())


@pytest.fixture(scope="module")
def shingles(workdir, gpu_available):
    return Case(E.write_scene(workdir, "multi_shingles"), *E.generic())


@pytest.fixture(scope="module")
def shingles_tr(workdir, gpu_available):
    return Case(E.write_scene(workdir, "multi_shingles_tr", transparent=True), *E.generic())


@pytest.fixture(scope="module")
def shingles_big(workdir, gpu_available):
    o, d = E.generic()
    return Case(E.write_scene(workdir, "multi_shingles_big", transparent=True, scale=E.BIG), o * F32(E.BIG), d * F32(E.BIG))


@pytest.fixture(scope="module")
def doubled(workdir, gpu_available):
    return Case(MH.write_doubled(workdir, "multi_doubled"), *E.generic())


def _multi(sc, o, d, stride, k, tmin=None, tmax=None, to_dest=False, count_all=False, count=None, n=None, stream=None):
    """One multi-hit query into sentinel-filled outputs: (records [cap, k, 4] uint32, nhits [cap] int32)."""
    n = len(o) if n is None else n
    cap = max(CAP, len(o) + 8)
    do, dd = _dev_rays(o[:n], d[:n], stride)
    rec = torch.full((cap, k, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    nh = torch.full((cap,), NH_SENTINEL, dtype=torch.int32, device=DEV)
    res = sc.multi_hit_device(do, dd, k, tmin=_dev(tmin), tmax=_dev(tmax), to_dest=to_dest, count_all=count_all, count=count,
                              out=(rec, nh), stream=stream)
    assert len(res) == 4 and res[0].shape == (n, k) and res[1].shape == (n, k) and res[2].shape == (n, k, 2) and res[3].shape == (n,)
    assert res[0].data_ptr() == rec.data_ptr() and res[3].data_ptr() == nh.data_ptr()
    assert res[0].dtype == res[3].dtype == torch.int32 and res[1].dtype == res[2].dtype == torch.float32
    return _np(rec).view(np.uint32), _np(nh)


def _check(got, want_rec, want_nh, live, what=""):
    rec, nh = got
    bad = np.flatnonzero((rec[:live] != want_rec[:live]).any(axis=(1, 2)))
    assert bad.size == 0, f"{what}: {bad.size} rays differ, first {bad[:4]}: {rec[bad[:2]]} for {want_rec[bad[:2]]}"
    assert np.array_equal(nh[:live], want_nh[:live]), f"{what}: nhits differ at {np.flatnonzero(nh[:live] != want_nh[:live])[:8]}"
    assert (rec[live:].view(np.int32) == REC_SENTINEL).all() and (nh[live:] == NH_SENTINEL).all(), f"{what}: rows past {live} written"


def _check_case(case, sc, k, name, kw, what, strides=(3,), count_all=(False,)):
    """One range case at one k against the helper, without and / or with RT_MULTI_COUNT_ALL; returns the totals."""
    rec, nh, m = case.first_k(k, name, **kw)
    n = len(case.o)
    for stride in strides:
        for ca in count_all:
            got = _multi(sc, case.o, case.d, stride, k, count_all=ca, **kw)
            _check(got, rec, m if ca else nh, n, f"{what}, {name}, k {k}, count_all {ca}, stride {stride}")
    return m


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "qo", "shingles", "shingles_tr"])
def test_k_one_is_the_closest_record_entry(which, request):
    case = request.getfixturevalue(which)
    n = len(case.o)
    with R.Scene.load(case.path, device=0) as sc:
        for name, kw in case.menu().items():
            want = case.closest(**kw)
            for stride in STRIDES:
                do, dd = _dev_rays(case.o, case.d, stride)
                tri, dist, st = sc.closest_hit_device(do, dd, tmin=_dev(kw.get("tmin")), tmax=_dev(kw.get("tmax")),
                                                      to_dest=kw.get("to_dest", False))
                theirs = _np(tri.unsqueeze(1).repeat(1, 4))                    # the same scene object's records
                theirs[:, 1] = _np(dist.contiguous().view(torch.int32))
                theirs[:, 2:] = _np(st.contiguous().view(torch.int32))
                rec, nh = _multi(sc, case.o, case.d, stride, 1, **kw)
                assert np.array_equal(rec[:n, 0].view(np.int32), theirs), f"{which}, {name}, stride {stride}"
                _check((rec, nh), want["record"][:, None, :], (want["triangle"] >= 0).astype(np.int32), n, f"{which}, {name}, stride {stride}")
        # the tensors the call allocates, and their views
        do, dd = _dev_rays(case.o, case.d, 3)
        tri, dist, st, nh = sc.multi_hit_device(do, dd, 1)
        want = case.closest()
        assert tri.shape == (n, 1) and dist.shape == (n, 1) and st.shape == (n, 1, 2) and nh.shape == (n,)
        assert np.array_equal(_np(tri)[:, 0], want["triangle"]) and np.array_equal(_np(dist).view(np.uint32)[:, 0], want["record"][:, 1])
        assert np.array_equal(_np(st.contiguous()).view(np.uint32)[:, 0], want["record"][:, 2:])


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shingles", "q"])
def test_every_k(which, request):
    case = request.getfixturevalue(which)
    classes = set()
    with R.Scene.load(case.path, device=0) as sc:
        for k in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16):
            for name, kw in case.short_menu().items():
                m = _check_case(case, sc, k, name, kw, which)
                classes |= {c for c, have in (("none", (m == 0).any()), ("short", ((m > 0) & (m < k)).any()), ("exact", (m == k).any()),
                                              ("truncated", (m > k).any())) if have}
                if which == "shingles" and name == "half-line" and k == KMAX:
                    assert (m > k).sum() >= 20 and ((m > 0) & (m < k)).sum() >= 20 and (m == 0).sum() >= 20
    assert classes == {"none", "short", "exact", "truncated"}


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["bvh", "brute_force"])
def test_ties_keep_the_lowest_indices(doubled, accel):
    case = doubled
    full, _, m = case.first_k(int(3 * 36), "full")
    assert m.max() == 108 and (m >= 3 * KMAX).any()
    hit = m > 0
    run = full[hit, :3]
    assert (run[:, 0, 1] == run[:, 1, 1]).all() and (run[:, 1, 1] == run[:, 2, 1]).all()          # three at the closest distance
    assert (run[:, 0, 0] < E.N_TRI).all() and (run[:, 1, 0] == run[:, 0, 0] + E.N_TRI).all()
    with R.Scene.load(case.path, device=0) as sc:
        sc.set_accel(accel)
        assert sc.accel() == accel
        for k in (1, 2, 3, 4, 16):
            for name in ("half-line", "tmin = second", "second to third"):
                _check_case(case, sc, k, name, case.short_menu()[name], "doubled, " + accel, strides=STRIDES if k == 4 else (3,))
            rec, nh, _ = case.first_k(k, "half-line")
            assert np.array_equal(rec, full[:, :k])                            # k = 2, 4: cut inside a run of three
            assert (rec[hit, 0, 0] < E.N_TRI).all()                           # k = 1: the lowest copy
        # closest_hit_device stepped by nextafter finds the lowest copy only; the list has all three
        do, dd = _dev_rays(case.o, case.d, 3)
        tri, dist, _ = sc.closest_hit_device(do, dd)
        tri2, _, _ = sc.closest_hit_device(do, dd, tmin=torch.nextafter(dist, torch.full_like(dist, float("inf"))))
        t1, t2 = _np(tri), _np(tri2)
        assert np.array_equal(t1[hit].astype(np.uint32), full[hit, 0, 0]) and (t2[hit] != t1[hit] + E.N_TRI).all()


# 4 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shingles", "doubled", "shingles_tr"])
def test_count_all(which, request):
    case = request.getfixturevalue(which)
    n = len(case.o)
    with R.Scene.load(case.path, device=0) as sc:
        for k in (1, 4, 16):
            for name, kw in case.menu().items():
                rec, nh, m = case.first_k(k, name, **kw)
                plain = _multi(sc, case.o, case.d, 3, k, **kw)
                flagged = _multi(sc, case.o, case.d, 3, k, count_all=True, **kw)
                _check(plain, rec, np.minimum(m, k), n, f"{which}, {name}, k {k}")
                _check(flagged, rec, m, n, f"{which}, {name}, k {k}, count all")
                assert plain[0].tobytes() == flagged[0].tobytes()              # the hit rows: the same bytes
            if k == 1:
                assert (case.first_k(1, "half-line")[2] > 1).sum() >= 100       # counts the flag alone can report


# 5 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "shingles_tr"])
def test_every_traversal_gives_the_same_bytes(which, request):
    case = request.getfixturevalue(which)
    menu = case.short_menu()
    with R.Scene.load(case.path, device=0) as sc:
        assert sc.accel() == "bvh"

        def run(what):
            for k in (3, 16):
                for name, kw in menu.items():
                    _check_case(case, sc, k, name, kw, f"{which}, {what}", count_all=(False, True))

        run("four-wide")
        sc.tune("lds_stack", 1)                                 # every push beyond the first through the overflow path:
        run("four-wide, lds_stack 1")                           # no subtree may be walked twice (lists, counts)
        sc.tune("lds_stack", 16)
        sc.set_profiling(True, count_work=True)                 # the counting instantiations
        sc.reset_stats()
        run("four-wide, counting")
        assert sc.work_stats(_capi.KERNEL_CLOSEST_HIT)[1] > 0
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
    """Shingles times 2^21 (scene_m1 >= 1e6: the binary tree whatever bvh_width says)."""
    case = shingles_big
    assert (case.first_k(3, "half-line")[2] > 3).sum() >= 100
    with R.Scene.load(case.path, device=0) as sc:
        assert np.abs(sc.export()["vertices"]).sum(axis=1).max() >= 1e6
        for k in (3, 16):
            for name, kw in case.short_menu().items():
                _check_case(case, sc, k, name, kw, "scaled", strides=(4,), count_all=(False, True))


# 6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_prefixes_by_n_and_by_device_count(q, stride):
    k = 3
    two = (F32(2) * q.len).astype(F32)
    rec, nh, m = q.first_k(k, "twice the length", tmax=two)
    assert [int((m[:n] > 0).sum()) for n in QS.PREFIXES] == [1, 63, 64, 65, 123, 157]
    n_all = len(q.o)
    with R.Scene.load(q.path, device=0) as sc:
        for n in QS.PREFIXES:
            _check(_multi(sc, q.o, q.d, stride, k, tmax=two[:n], n=n), rec, nh, n, f"n {n}")
        for count, live in [(c, c) for c in QS.PREFIXES] + [(-5, 0), (0, 0), (n_all + 7, n_all)]:
            cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
            _check(_multi(sc, q.o, q.d, stride, k, tmax=two, count=cnt), rec, nh, live, f"count {count}")
            _check(_multi(sc, q.o, q.d, stride, k, tmax=two, count=cnt, count_all=True), rec, m, live, f"count {count}, count all")
            # outputs the call allocates: rows past the live count hold the miss record and 0
            do, dd = _dev_rays(q.o, q.d, stride)
            tri, dist, st, cnts = sc.multi_hit_device(do, dd, k, tmax=_dev(two), count=cnt)
            assert np.array_equal(_np(tri)[:live].astype(np.uint32), rec[:live, :, 0]) and (_np(tri)[live:] == -1).all()
            assert (_np(dist).view(np.uint32)[live:] == RR.INF_BITS).all() and (_np(st.contiguous()).view(np.uint32)[live:] == 0).all()
            assert np.array_equal(_np(cnts)[:live], nh[:live]) and (_np(cnts)[live:] == 0).all()


# 7 -------------------------------------------------------------------------------------------------
def test_mixed_lanes_in_one_wave(shingles):
    """128 rays in one launch: ray i takes menu entry i mod 8 as explicit bounds, every fifth an empty range."""
    case = shingles
    n, k = 128, 4
    nan = F32(np.nan)
    empties = [dict(tmin=nan), dict(tmax=nan), dict(tmax=F32(0)), dict(tmax=F32(-1)), dict(tmin=F32(5), tmax=F32(1)), dict(tmin=F32(1), tmax=F32(1))]
    tmin, tmax = np.zeros(len(case.o), F32), np.full(len(case.o), np.inf, F32)
    for j, kw in enumerate(case.menu().values()):
        rows = np.arange(len(case.o)) % 8 == j
        if kw.get("to_dest"):
            tmax[rows] = case.len[rows]
        if kw.get("tmin") is not None:
            tmin[rows] = kw["tmin"][rows]
        if kw.get("tmax") is not None:
            tmax[rows] = kw["tmax"][rows]
    empty = np.arange(len(case.o)) % 5 == 4
    for i in np.flatnonzero(empty):
        kind = empties[(i // 5) % len(empties)]
        tmin[i], tmax[i] = kind.get("tmin", F32(0)), kind.get("tmax", INF)
    rec, nh, m = case.first_k(k, None, tmin=tmin, tmax=tmax)
    mm = m[:n]
    assert (mm[empty[:n]] == 0).all() and (mm[~empty[:n]] == 0).sum() >= 10           # empty ranges; misses
    assert ((mm > 0) & (mm < k)).sum() >= 10 and (mm > k).sum() >= 20                       # short and truncated lists
    for w in (slice(0, 64), slice(64, 128)):                                          # ... in each wave
        assert (mm[w] == 0).any() and ((mm[w] > 0) & (mm[w] < k)).any() and (mm[w] > k).any()
    with R.Scene.load(case.path, device=0) as sc:
        for stride in STRIDES:
            for ca in (False, True):
                got = _multi(sc, case.o, case.d, stride, k, tmin=tmin[:n], tmax=tmax[:n], count_all=ca, n=n)
                _check(got, rec, m if ca else nh, n, f"mixed, stride {stride}, count_all {ca}")


# 8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ["B", "C"])
def test_long_and_short_rays(shingles_tr, letter):
    """Class B (dot(dir, dir) overflows: the walks' distance cull is off; the longest meet every triangle) and C
    (short), k = 4, with finite bounds from the helper."""
    o, d, where = E.class_rays(letter)
    case = Case(shingles_tr.path, o, d, shingles_tr.T, shingles_tr.transparent)
    hit = case.d1 < INF
    assert hit.sum() >= (3 if letter == "B" else 2) * 150
    menu = {"below the third": dict(tmax=case.d3), "second to third": dict(tmin=case.d2, tmax=case.d3), "to dest": dict(to_dest=True),
            "half-line": dict()}
    with R.Scene.load(case.path, device=0) as sc:
        for width in (4, 2):
            sc.tune("bvh_width", width)
            for name, kw in menu.items():
                m = _check_case(case, sc, 4, name, kw, f"class {letter}, width {width}", count_all=(False, True))
                if name == "half-line":
                    assert (m > 4).sum() >= 300
                if name == "below the third":
                    assert (m[hit] >= 1).all() and (m <= 2).all()


# 9 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(q):
    """A query queued before update_vertices answers for the old vertices, one queued after it for the new."""
    st = torch.cuda.Stream(device=DEV)
    k, reps, n = 3, 16, len(q.o)
    two = (F32(2) * q.len).astype(F32)
    old_rec, old_nh, _ = q.first_k(k, "twice the length", tmax=two)
    with R.Scene.load(q.path, device=0) as sc:
        e = sc.export()
        new = S.deform(e["vertices"], 0.03)
        moved = Case(q.path, q.o, q.d, np.ascontiguousarray(new[e["triangles"].astype(np.int64)], F32), q.transparent)
        new_rec, new_nh, new_m = moved.first_k(k, None, tmax=two)
        assert not np.array_equal(new_rec, old_rec)
        with torch.cuda.stream(st):
            do, dd = _dev_rays(q.o, q.d, 3)
            bo, bd, bt = do.repeat(reps, 1), dd.repeat(reps, 1), _dev(two).repeat(reps)
            tri, dist, sts, nh = sc.multi_hit_device(bo, bd, k, tmax=bt)
        assert sc.update_vertices(new) == "refit"
        with torch.cuda.stream(st):
            tri2, dist2, sts2, nh2 = sc.multi_hit_device(do, dd, k, tmax=_dev(two), count_all=True)
        st.synchronize()
        u32 = lambda t: _np(t.contiguous()).view(np.uint32)
        assert np.array_equal(u32(tri).reshape(reps, n, k), np.tile(old_rec[:, :, 0], (reps, 1, 1)))
        assert np.array_equal(u32(dist).reshape(reps, n, k), np.tile(old_rec[:, :, 1], (reps, 1, 1)))
        assert np.array_equal(u32(sts).reshape(reps, n, k, 2), np.tile(old_rec[:, :, 2:], (reps, 1, 1, 1)))
        assert np.array_equal(_np(nh).reshape(reps, n), np.tile(old_nh, (reps, 1)))
        assert np.array_equal(u32(tri2), new_rec[:, :, 0]) and np.array_equal(u32(dist2), new_rec[:, :, 1])
        assert np.array_equal(u32(sts2), new_rec[:, :, 2:]) and np.array_equal(_np(nh2), new_m)


# 10 ------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(q):
    """Each RT_E_ARG case alone on a scene with a device; nothing is written."""
    L = _capi.lib()
    k = 4
    do, dd = _dev_rays(q.o[:8], q.d[:8], 4)
    rec = torch.full((CAP, k, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    nh = torch.full((CAP,), NH_SENTINEL, dtype=torch.int32, device=DEV)
    tb = torch.ones(CAP, dtype=torch.float32, device=DEV)
    cnt = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with R.Scene.load(q.path, device=0) as sc:
        h = sc.handle
        good = dict(o=vp(do), d=vp(dd), stride=4, n=8, count=vp(cnt), tmin=vp(tb), tmax=vp(tb, 64), flags=_capi.RANGE_TO_DEST, k=k,
                    out=vp(rec), nh=vp(nh))

        def call(**kw):
            a = dict(good, **kw)
            return L.rt_multi_hit_range_device(h, a["o"], a["d"], a["stride"], a["n"], a["count"], a["tmin"], a["tmax"], a["flags"],
                                               a["k"], a["out"], a["nh"], None)

        cases = [dict(n=-1), dict(stride=5), dict(d=None), dict(o=vp(do, 4), n=7), dict(count=vp(cnt, 2)), dict(tmin=vp(tb, 1)),
                 dict(tmax=vp(tb, 2)), dict(flags=1 << 3), dict(flags=(1 << 31) | 1), dict(flags=_capi.OCCLUDE_ANY_OPAQUE),
                 dict(flags=_capi.OCCLUDE_ANY_OPAQUE | _capi.RANGE_TO_DEST),
                 dict(k=0), dict(k=-1), dict(k=KMAX + 1), dict(out=None), dict(out=vp(rec, 8)), dict(out=vp(rec, 4)), dict(nh=vp(nh, 2)),
                 dict(flags=_capi.MULTI_COUNT_ALL, nh=None), dict(n=(2 ** 31 - 1) // k + 1)]
        for kw in cases:
            assert call(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        assert call(n=0, o=None, d=None, out=None, nh=None) == _capi.RT_OK          # n == 0: nothing to do
        torch.cuda.synchronize()
        assert (_np(rec) == REC_SENTINEL).all() and (_np(nh) == NH_SENTINEL).all()   # nothing was written
        assert call(nh=None) == _capi.RT_OK                                         # nhits may be NULL without the flag
        torch.cuda.synchronize()
        want = q.first_k(k, None, tmin=np.ones(len(q.o), F32), tmax=np.ones(len(q.o), F32))[0]
        assert np.array_equal(_np(rec).view(np.uint32)[:8], want[:8]) and (_np(nh) == NH_SENTINEL).all()
        # the Python forms
        for bad in (dict(tmin=tb.cpu()), dict(tmax=tb[:4]), dict(out=rec), dict(out=(rec[:4], nh)), dict(out=(rec, nh[:4])),
                    dict(out=(rec[:, :2], nh)), dict(count=torch.zeros(1, dtype=torch.int32))):
            with pytest.raises(ValueError):
                sc.multi_hit_device(do, dd, k, **bad)
        with pytest.raises(ValueError):
            sc.multi_hit_device(do, dd, KMAX + 1)
        e_tri, e_dist, e_st, e_nh = sc.multi_hit_device(do[:0], dd[:0], k)
        assert e_tri.shape == (0, k) and e_dist.shape == (0, k) and e_st.shape == (0, k, 2) and e_nh.shape == (0,)
