"""Inside and signed-distance queries (rt_point_inside_device, rt_signed_distance_device: k_bvh_inside, k_inside):
per query point the number of candidate triangles the half line along a coordinate axis crosses, its parity, and
the closest-point record with that parity as the distance's sign; points and results in torch CUDA tensors.

The expectation is tests/_inside_ref.py, the numpy restatement of the definition in include/raytracert.h, which
tests/test_inside_ref.py checks on the CPU against a float64 winding number. Equality is of bytes throughout: there
is no tolerance. The meshes are indexed (shared vertices): the cube, the blob, the nested blob, the open blob and
the blob with zero-area and edge-on triangles; the points are the cube's grid, points exactly under vertices and
1,024 uniform points, the smallest sets that put shared edges and vertices under points in projection.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import raytracert_amd as R
from raytracert_amd import _capi

import _inside_ref as IR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
IN_SENTINEL = 0xAB
CR_SENTINEL = -9
REC_SENTINEL = -7
NAN_SENTINEL = 0x7FC0DEAD      # a NaN bit pattern no kernel computes
STRIDES = (3, 4)
INF_BITS, SIGN = 0x7F800000, 0x80000000
BUILDERS = ("sah", "lbvh", "cluster")


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


class Case:
    """A mesh, its points and the restatement's crossings per axis, each computed once and never changed."""

    def __init__(self, name, V=None, tri=None, p=None):
        self.name = name
        if V is None:
            V, tri = IR.MESHES[name]()
        self.V, self.tri = np.ascontiguousarray(V, F32), np.ascontiguousarray(tri, np.uint32)
        self.p = IR.mesh_points(name, self.V) if p is None else p
        self._want = {}

    def want(self, axis):
        if axis not in self._want:
            cr = IR.crossings(self.p, self.V, self.tri, axis)
            cr.setflags(write=False)
            self._want[axis] = cr
        return self._want[axis]

    def create(self, builder="sah"):
        return R.Scene.create(self.V, self.tri, np.zeros(len(self.tri), np.uint32), IR.MATERIALS, device=0, builder=builder)


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module")
def blob(gpu_available):
    return _case("blob")


@pytest.fixture(scope="module")
def nested(gpu_available):
    return _case("nested")


def _query(sc, p, axis, stride=3, count=None, n=None, crossings=True, stream=None):
    """One query into sentinel-filled outputs: (inside [cap] uint8, crossings [cap] int32)."""
    n = len(p) if n is None else n
    cap = len(p) + 8
    ins = torch.full((cap,), IN_SENTINEL, dtype=torch.uint8, device=DEV)
    cr = torch.full((cap,), CR_SENTINEL, dtype=torch.int32, device=DEV)
    res = sc.point_inside_device(_dev_points(p[:n], stride), axis=axis, crossings=crossings, count=count,
                                 out=(ins, cr) if crossings else ins, stream=stream)
    if crossings:
        assert res[0].shape == (n,) and res[0].dtype == torch.uint8 and res[0].data_ptr() == ins.data_ptr()
        assert res[1].shape == (n,) and res[1].dtype == torch.int32 and res[1].data_ptr() == cr.data_ptr()
    else:
        assert res.shape == (n,) and res.dtype == torch.uint8 and res.data_ptr() == ins.data_ptr()
    return _np(ins), _np(cr)


def _check(got, want, live, what="", crossings=True):
    ins, cr = got
    want = np.asarray(want)
    if crossings:
        bad = np.flatnonzero(cr[:live] != want[:live])
        assert bad.size == 0, f"{what}: the crossings of {bad.size} points differ, first points {bad[:5]}: {cr[bad[:5]]} for {want[bad[:5]]}"
        assert (cr[live:] == CR_SENTINEL).all(), f"{what}: crossings past {live} written"
    else:
        assert (cr == CR_SENTINEL).all(), f"{what}: crossings written without being asked for"
    assert np.array_equal(ins[:live], IR.inside(want[:live])), f"{what}: verdicts differ at {np.flatnonzero(ins[:live] != IR.inside(want[:live]))[:5]}"
    assert (ins[live:] == IN_SENTINEL).all(), f"{what}: verdicts past {live} written"


def _all_axes(sc, case, what, strides=STRIDES, counted=True):
    n = len(case.p)
    for axis, stride in itertools.product(IR.AXES, strides):
        w = f"{case.name}, {what}, axis {IR.AXIS_NAMES[axis]}, stride {stride}"
        _check(_query(sc, case.p, axis, stride), case.want(axis), n, w)
        if counted:
            cnt = torch.tensor([n - 7], dtype=torch.int32, device=DEV)
            _check(_query(sc, case.p, axis, stride, count=cnt, crossings=(axis & 1) == 0), case.want(axis), n - 7, w + ", d_count",
                   crossings=(axis & 1) == 0)


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cube", "blob", "nested", "open", "degenerate"])
def test_meshes_against_the_restatement(which, gpu_available):
    case = _case(which)
    assert len(case.p) >= 1024 + 300
    if which == "cube":
        interior, outside = IR.cube_grid_classes(case.p[:125])
        for axis in IR.AXES:
            assert (IR.inside(case.want(axis)[:125])[interior] == 1).all() and (case.want(axis)[:125][outside] % 2 == 0).all()
    if which == "nested":
        assert max(case.want(a).max() for a in IR.AXES) >= 4
    with case.create() as sc:                                   # freshly created: no update has made the device vertices yet
        sc.bvh_validate()
        _all_axes(sc, case, "sah, width 4, fresh")
        sc.tune("bvh_width", 2)
        _all_axes(sc, case, "sah, width 2")
        sc.tune("bvh_width", 4)
        sc.tune("lds_stack", 1)                                 # every push beyond the first through the overflow path
        _all_axes(sc, case, "sah, lds_stack 1", strides=(3,), counted=False)
        sc.tune("lds_stack", 16)
        sc.set_accel("brute_force")
        _all_axes(sc, case, "brute force")
        sc.set_accel("bvh")
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(case.V, "rebuild") in ("rebuilt_lbvh", "rebuilt_" + builder)   # (a tiny mesh may hand over)
            sc.bvh_validate()
            for width in (4, 2):
                sc.tune("bvh_width", width)
                _all_axes(sc, case, f"{builder}, width {width}")
        sc.set_profiling(True, count_work=True)                 # the counting instantiations
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _all_axes(sc, case, f"cluster, width {width}, counting", counted=False)
        sc.set_profiling(False)
    # a scene whose first trees are the device builder's, queried before anything else
    with case.create(builder="lbvh") as sc:
        _all_axes(sc, case, "created with lbvh, fresh", strides=(4,), counted=False)


# 2 -------------------------------------------------------------------------------------------------
def test_after_updates_and_mesh_changes(blob, nested):
    """Every state the device vertices can be in: a host update, a device update (before and after a first query),
    set_mesh from device tensors, set_mesh to no triangles."""
    p, n = blob.p, len(blob.p)
    v1 = (blob.V * F32(1.1)).astype(F32)
    v2 = (blob.V * F32(0.8) + F32(0.05)).astype(F32)
    c1, c2 = Case("blob x 1.1", v1, blob.tri, p), Case("blob moved", v2, blob.tri, p)
    on_nested = Case("nested, the blob's points", nested.V, nested.tri, p)
    assert any(not np.array_equal(c1.want(a), blob.want(a)) for a in IR.AXES)
    axes = (4, 1, 2, 5)
    with blob.create() as sc:
        for axis in axes:
            _check(_query(sc, p, axis), blob.want(axis), n, f"fresh, axis {axis}")
        assert sc.update_vertices(v1) == "refit"                # host array
        for width in (4, 2):
            sc.tune("bvh_width", width)
            for axis in axes:
                _check(_query(sc, p, axis, 4), c1.want(axis), n, f"after the host update, width {width}, axis {axis}")
        assert sc.update_vertices(torch.from_numpy(v2).to(DEV)) == "refit"
        for width in (4, 2):
            sc.tune("bvh_width", width)
            for axis in axes:
                _check(_query(sc, p, axis, 3), c2.want(axis), n, f"after the device update, width {width}, axis {axis}")
        sc.set_accel("brute_force")
        _check(_query(sc, p, 4), c2.want(4), n, "after the device update, brute force")
        sc.set_accel("bvh")
        for builder in BUILDERS:
            sc.set_builder(builder)
            v = torch.from_numpy(nested.V).to(DEV)
            t = torch.from_numpy(nested.tri.view(np.int32)).to(DEV)
            m = torch.zeros(len(nested.tri), dtype=torch.int32, device=DEV)
            sc.set_mesh(v, t, m)
            for width in (4, 2):
                sc.tune("bvh_width", width)
                for axis in axes:
                    _check(_query(sc, p, axis, 3), on_nested.want(axis), n, f"after set_mesh_device ({builder}), width {width}, axis {axis}")
            sc.set_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32))
            for accel in ("bvh", "brute_force"):
                sc.set_accel(accel)
                for axis in (4, 3):
                    _check(_query(sc, p, axis, 4), np.zeros(n, np.int32), n, f"no triangles ({builder}, {accel})")
            sc.set_accel("bvh")
            sc.set_mesh(blob.V, blob.tri, np.zeros(len(blob.tri), np.uint32))      # host arrays: the blob again
            _check(_query(sc, p, 4), blob.want(4), n, f"the blob again ({builder})")
    # the first thing that happens to a fresh scene is a device update; then a refit from a host array
    with blob.create() as sc:
        assert sc.update_vertices(torch.from_numpy(v1).to(DEV)) == "refit"
        _check(_query(sc, p, 2), c1.want(2), n, "a device update first")
        assert sc.update_vertices(v2) == "refit"
        _check(_query(sc, p, 2), c2.want(2), n, "then a host update")
    # ... and a query first, then the first update: the refit finds its buffers half made and completes them
    with blob.create() as sc:
        _check(_query(sc, p, 0), blob.want(0), n, "a query first")
        assert sc.update_vertices(torch.from_numpy(v2).to(DEV)) == "refit"
        sc.bvh_validate()
        _check(_query(sc, p, 0), c2.want(0), n, "then the first update")
        assert sc.update_vertices(v1, "rebuild") == "rebuilt"
        _check(_query(sc, p, 0), c1.want(0), n, "then a rebuild")


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["blob", "nested"])
def test_signed_distance(which, request):
    case = request.getfixturevalue(which)
    p, n = case.p, len(case.p)
    finite = np.isfinite(p).all(axis=1)
    small = np.full(n, 0.05, F32)
    with case.create() as sc:
        for accel, stride, axis, rmax in (("bvh", 3, 4, None), ("bvh", 4, 1, small), ("brute_force", 3, 2, small), ("bvh", 3, 3, None)):
            sc.set_accel(accel)
            what = f"{which}, {accel}, stride {stride}, axis {axis}, rmax {'none' if rmax is None else 0.05}"
            dp = _dev_points(p, stride)
            rm = None if rmax is None else torch.from_numpy(rmax).to(DEV)
            rec0 = torch.full((n + 8, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
            pts0 = torch.full((n + 8, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            sc.closest_point_device(dp, rmax=rm, out=(rec0, pts0), want_points=True)
            rec = torch.full((n + 8, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
            pts = torch.full((n + 8, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            tri, dist, st, ins, cp = sc.signed_distance_device(dp, rmax=rm, axis=axis, out=(rec, pts), want_points=True)
            assert tri.shape == (n,) and dist.shape == (n,) and st.shape == (n, 2) and ins.shape == (n,) and cp.shape == (n, 3)
            assert tri.data_ptr() == rec.data_ptr() and cp.data_ptr() == pts.data_ptr() and ins.dtype == torch.uint8
            r, r0 = _np(rec).view(np.uint32), _np(rec0).view(np.uint32)
            want_in = IR.inside(case.want(axis))
            assert np.array_equal(_np(ins), want_in), what
            assert np.array_equal(r[:n, 1] >> 31, want_in), f"{what}: the sign bit is not the verdict"
            cleared = r.copy()
            cleared[:n, 1] &= ~np.uint32(SIGN)
            assert np.array_equal(cleared, r0), f"{what}: the records differ from the closest-point query's"
            assert np.array_equal(_bits(pts), _bits(pts0)), f"{what}: the points differ"
            assert (r[n:].view(np.int32) == REC_SENTINEL).all()
            assert (r[:n][~finite] == np.array([0xFFFFFFFF, INF_BITS, 0, 0], np.uint32)).all(), f"{what}: a non-finite point is a positive miss"
            miss = r0[:n, 0] == 0xFFFFFFFF
            if rmax is not None:                                 # a narrow band: misses keep the sign
                inside_miss, outside_miss = miss & (want_in == 1), miss & (want_in == 0)
                assert inside_miss.sum() >= 50 and outside_miss.sum() >= 50 and (~miss).sum() >= 10, what
                assert (r[:n, 1][inside_miss] == (INF_BITS | SIGN)).all() and (r[:n, 1][outside_miss] == INF_BITS).all(), what
                assert np.isneginf(_np(dist)[inside_miss]).all() and np.isposinf(_np(dist)[outside_miss]).all()
            else:
                assert not miss[finite].any()
                d = _np(dist)[finite]
                assert ((d < 0) == (want_in[finite] == 1)).all() and (want_in[finite] == 1).sum() >= 100
        # without the optional outputs, through the C entry: the records alone
        sc.set_accel("bvh")
        dp = _dev_points(p, 3)
        rec2 = torch.full((n, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
        rc = _capi.lib().rt_signed_distance_device(sc.handle, C.c_void_p(dp.data_ptr()), 3, n, None, None, 3, 0, C.c_void_p(rec2.data_ptr()),
                                                   None, None, None)
        assert rc == _capi.RT_OK
        torch.cuda.synchronize()
        assert np.array_equal(_np(rec2).view(np.uint32), r[:n])


# 4 -------------------------------------------------------------------------------------------------
def test_the_walk_culls(blob):
    """With RT_PROFILE_WORK on the blob, 1,024 uniform points: the triangle evaluations per point stay below
    nt / 4 on every builder and width (a cap, not a measurement: tests/test_inside_ref.py shows that the columns
    themselves hold fewer than nt / 16 triangles; the loop over every triangle evaluates nt)."""
    p = IR.uniform_points(blob.V, 1024, 60)
    n, nt = len(p), len(blob.tri)
    case = Case("blob, uniform", blob.V, blob.tri, p)
    with blob.create() as sc:
        sc.set_profiling(True, count_work=True)
        for builder in BUILDERS:
            sc.set_builder(builder)
            sc.update_vertices(blob.V, "rebuild")
            for width, axis in itertools.product((4, 2), (4, 1)):
                sc.tune("bvh_width", width)
                sc.reset_stats()
                _check(_query(sc, p, axis), case.want(axis), n, f"{builder}, width {width}, axis {axis}")
                tests, visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                print(f"{builder}, width {width}, axis {IR.AXIS_NAMES[axis]}: {tests / n:.2f} evaluations, {visits / n:.2f} node visits per point "
                      f"({nt} triangles)")
                assert 0 < tests / n < nt / 4 and visits > 0, f"{builder}, width {width}, axis {axis}: {tests / n:.2f} evaluations per point"
        sc.set_profiling(False)


# 5 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(blob):
    """Queries queued on two streams before update_vertices answer for the old vertices, those queued after it for
    the new."""
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    reps, p, n = 16, blob.p, len(blob.p)
    v1 = (blob.V * F32(1.1)).astype(F32)
    moved = Case("blob x 1.1", v1, blob.tri, p)
    old, now = blob.want(4), moved.want(4)
    assert (old != now).sum() >= 50
    with blob.create() as sc:
        with torch.cuda.stream(s1):
            dp = _dev_points(p, 3)
            ins1, cr1 = sc.point_inside_device(dp.repeat(reps, 1), axis=4, crossings=True)      # (the current stream: s1)
        s1.synchronize()                                        # (dp is made; the second stream only reads it)
        with torch.cuda.stream(s2):
            sd = sc.signed_distance_device(dp.repeat(reps, 1), axis=4, stream=s2)
        assert sc.update_vertices(v1) == "refit"
        with torch.cuda.stream(s1):
            ins2, cr2 = sc.point_inside_device(dp, axis=4, crossings=True, stream=s1)
        with torch.cuda.stream(s2):
            sd2 = sc.signed_distance_device(dp, axis=4, stream=s2)
        s1.synchronize()
        s2.synchronize()
        assert np.array_equal(_np(cr1).reshape(reps, n), np.tile(old, (reps, 1)))
        assert np.array_equal(_np(ins1).reshape(reps, n), np.tile(IR.inside(old), (reps, 1)))
        assert np.array_equal(_np(sd[3]).reshape(reps, n), np.tile(IR.inside(old), (reps, 1)))
        assert np.array_equal((_bits(sd[1]) >> 31).reshape(reps, n), np.tile(IR.inside(old), (reps, 1)))
        assert np.array_equal(_np(cr2), now) and np.array_equal(_np(ins2), IR.inside(now))
        assert np.array_equal(_np(sd2[3]), IR.inside(now)) and np.array_equal(_bits(sd2[1]) >> 31, IR.inside(now))
        tri_old, tri_new = _np(sd[0]).reshape(reps, n), _np(sd2[0])
        assert (tri_old == tri_old[0]).all()
        rec = sc.closest_point_device(dp)
        assert np.array_equal(tri_new, _np(rec[0]))


# 6 -------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(blob):
    """Each RT_E_ARG case alone on a scene with a device; nothing is written."""
    L = _capi.lib()
    dp = _dev_points(blob.p[:8], 4)
    ins = torch.full((16,), IN_SENTINEL, dtype=torch.uint8, device=DEV)
    cr = torch.full((16,), CR_SENTINEL, dtype=torch.int32, device=DEV)
    rec = torch.full((16, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    pts = torch.full((16, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    rb = torch.ones(16, dtype=torch.float32, device=DEV)
    cnt = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with blob.create() as sc:
        good = dict(p=vp(dp), stride=4, n=8, count=vp(cnt), rmax=vp(rb), axis=4, flags=0, ins=vp(ins), cr=vp(cr), out=vp(rec), out2=vp(pts))

        def inside(**kw):
            a = dict(good, **kw)
            return L.rt_point_inside_device(sc.handle, a["p"], a["stride"], a["n"], a["count"], a["axis"], a["flags"], a["ins"], a["cr"], None)

        def signed(**kw):
            a = dict(good, **kw)
            return L.rt_signed_distance_device(sc.handle, a["p"], a["stride"], a["n"], a["count"], a["rmax"], a["axis"], a["flags"],
                                               a["out"], a["out2"], a["ins"], None)

        shared = [dict(n=-1), dict(stride=5), dict(stride=0), dict(p=None), dict(p=vp(dp, 4), n=7), dict(stride=3, p=vp(dp, 2)),
                  dict(count=vp(cnt, 2)), dict(flags=1), dict(flags=1 << 31), dict(flags=_capi.NEAR_COUNT_ALL), dict(axis=-1), dict(axis=6)]
        for kw in shared + [dict(ins=None), dict(cr=vp(cr, 2))]:
            assert inside(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        for kw in shared + [dict(out=None), dict(out=vp(rec, 8)), dict(out2=vp(pts, 2)), dict(rmax=vp(rb, 1))]:
            assert signed(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        assert inside(n=0, p=None, ins=None, cr=None) == _capi.RT_OK            # n == 0: nothing to do
        assert signed(n=0, p=None, out=None, out2=None, ins=None) == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(ins) == IN_SENTINEL).all() and (_np(cr) == CR_SENTINEL).all()
        assert (_np(rec) == REC_SENTINEL).all() and (_bits(pts) == NAN_SENTINEL).all()          # nothing was written
        assert inside() == _capi.RT_OK and inside(cr=None) == _capi.RT_OK
        assert signed() == _capi.RT_OK and signed(out2=None, ins=None, rmax=None, count=None) == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(ins)[:8] <= 1).all() and (_np(ins)[8:] == IN_SENTINEL).all()
        assert (_np(cr)[:8] >= 0).all() and (_np(cr)[8:] == CR_SENTINEL).all()
        assert (_np(rec)[:8, 0] != REC_SENTINEL).all() and (_np(rec)[8:] == REC_SENTINEL).all()
        assert (_bits(pts)[:8] != NAN_SENTINEL).all() and (_bits(pts)[8:] == NAN_SENTINEL).all()
        for kw in (dict(out=ins[:4]), dict(out=cr), dict(out=(ins, cr)), dict(out=ins, crossings=True), dict(out=(ins, cr[:4]), crossings=True),
                   dict(count=torch.tensor([8], dtype=torch.int64, device=DEV)), dict(axis=6)):
            with pytest.raises(ValueError):
                sc.point_inside_device(dp, **kw)
        for kw in (dict(rmax=torch.ones(4, dtype=torch.float32, device=DEV)), dict(out=rec[:4]), dict(out=rec, want_points=True), dict(axis=-1)):
            with pytest.raises(ValueError):
                sc.signed_distance_device(dp, **kw)
        assert sc.point_inside_device(torch.zeros((0, 3), dtype=torch.float32, device=DEV)).shape == (0,)
        assert sc.signed_distance_device(torch.zeros((0, 4), dtype=torch.float32, device=DEV))[3].shape == (0,)
