"""Triangle-distance queries (rt_triangle_distance_device, rt_triangle_within_device: k_bvh_tri_dist, k_tri_dist): per
query triangle the candidate triangle nearest to it below the query's radius, as the closest-point record with the
witness points on the query and on the scene, and whether there is one; queries and results in torch CUDA tensors
(Scene.triangle_distance, Scene.triangle_within).

The expectation is tests/_triangle_distance_ref.py, the numpy restatement of the definition in include/raytracert.h,
which tests/test_triangle_distance_ref.py checks on the CPU against an exact rational distance. Equality is of bytes
throughout: there is no tolerance. Outputs are filled with sentinels first, so rows past the live count are shown to
be untouched. The meshes are tests/_box_overlap_ref.py's (cube, blob, nested, open, degenerate, and the blob with a
sliver on the always list); the queries of a mesh are _triangle_distance_ref.distance_queries: the overlap tests'
mesh_queries (of which at least 300 overlap something), 400 of them shrunk and shifted off the surface, 40 shrunk
scene triangles lifted off along their normal, and with them the non-finite and the zero-area queries. A mesh's
expectation is computed once and never changed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import raytracert_amd as R
from raytracert_amd import _capi

import _inside_ref as IR
import _query_scenes as Q
import _triangle_distance_ref as DR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
REC_SENTINEL = -7
PT_SENTINEL = 12345.0
W_SENTINEL = 0xAB
STRIDES = (3, 4)
BUILDERS = ("sah", "lbvh", "cluster")


def _np(t):
    return t.cpu().numpy()


def _dev_tris(q, stride, junk):
    """Query triangles as a CUDA tensor in either layout; the padded layout's w holds values that must not matter."""
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    if stride == 4:
        w = np.where(np.arange(3 * len(q)) % 2 == 0, np.nan, junk).astype(F32).reshape(-1, 3, 1)
        q = np.concatenate([q, w], axis=2)
    return torch.from_numpy(np.ascontiguousarray(q)).to(DEV)


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


class Case:
    """A mesh, its queries, an optional self index per query, a radius per query, and the restatement's answers
    without and with the radii, computed once and never changed."""

    def __init__(self, name, V=None, tri=None, queries=None, self_index=None):
        self.name = name
        if V is None:
            V, tri = DR.MESHES[name]()
        self.V, self.tri = np.ascontiguousarray(V, F32), np.ascontiguousarray(tri, np.uint32)
        self.q = DR.distance_queries(self.V, self.tri) if queries is None else np.ascontiguousarray(queries, F32)
        self.n = len(self.q)
        self.self_index = None if self_index is None else np.ascontiguousarray(self_index, np.int32)
        self._matrix = None
        self._want = {}

    @property
    def matrix(self):
        if self._matrix is None:
            self._matrix = DR.dist2_matrix(self.q, self.V, self.tri)
            for a in self._matrix:
                a.setflags(write=False)
        return self._matrix

    @property
    def rmax(self):
        """Half the distance for every other query that has one, twice it for the rest; a small radius where the
        distance is 0, 1 where nothing is found, and a NaN, a zero and a negative radius now and then."""
        d = self.want(False)[0][:, 1].view(F32)
        with np.errstate(all="ignore"):
            r = np.where(np.arange(self.n) % 2 == 0, F32(0.5), F32(2.0)) * d
        r = np.where(d == 0, F32(0.01), np.where(np.isfinite(d), r, F32(1.0))).astype(F32)
        r[5::51], r[6::51], r[7::51] = np.nan, 0.0, -1.0
        return r

    def want(self, radii: bool):
        """(records [n, 4] int32, qpoints, points, within [n] uint8, eligible [n, nt], D2)."""
        if radii not in self._want:
            res = DR.answers(self.q, self.V, self.tri, rmax=self.rmax if radii else None, self_index=self.self_index, matrix=self.matrix)
            for a in res:
                a.setflags(write=False)
            self._want[radii] = res
        return self._want[radii]

    def create(self, builder="sah"):
        return R.Scene.create(self.V, self.tri, np.zeros(len(self.tri), np.uint32), DR.MATERIALS, device=0, builder=builder)


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module")
def blob(gpu_available):
    return _case("blob")


def _distance(sc, case, stride=3, radii=False, count=None, n=None, points=True, stream=None):
    """One record query into sentinel-filled outputs: (records [cap, 4] int32, qpoints [cap, 3], points [cap, 3])."""
    n = case.n if n is None else n
    cap = case.n + 8
    rec = torch.full((cap, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
    qp = torch.full((cap, 3), PT_SENTINEL, dtype=torch.float32, device=DEV)
    pp = torch.full((cap, 3), PT_SENTINEL, dtype=torch.float32, device=DEV)
    res = sc.triangle_distance(_dev_tris(case.q[:n], stride, 123.0), rmax=_dev(case.rmax[:n], F32) if radii else None,
                               self_index=_dev(None if case.self_index is None else case.self_index[:n], np.int32), count=count,
                               want_points=points, out=(rec, qp, pp) if points else rec, stream=stream)
    assert len(res) == (5 if points else 3) and res[0].shape == (n,) and res[0].dtype == torch.int32 and res[0].data_ptr() == rec.data_ptr()
    assert res[1].dtype == torch.float32 and res[2].shape == (n, 2)
    if points:
        assert res[3].data_ptr() == qp.data_ptr() and res[4].data_ptr() == pp.data_ptr() and res[4].shape == (n, 3)
    return _np(rec), _np(qp), _np(pp)


def _within(sc, case, stride=3, radii=True, count=None, n=None, stream=None):
    n = case.n if n is None else n
    w = torch.full((case.n + 8,), W_SENTINEL, dtype=torch.uint8, device=DEV)
    res = sc.triangle_within(_dev_tris(case.q[:n], stride, np.inf), rmax=_dev(case.rmax[:n], F32) if radii else None,
                             self_index=_dev(None if case.self_index is None else case.self_index[:n], np.int32), count=count, out=w,
                             stream=stream)
    assert res.shape == (n,) and res.dtype == torch.uint8 and res.data_ptr() == w.data_ptr()
    return _np(w)


def _check(got, want, live, what="", points=True):
    rec, qp, pp = got
    wrec, wqp, wpp = want[:3]
    bad = np.flatnonzero((rec[:live] != wrec[:live]).any(axis=1))
    assert bad.size == 0, (f"{what}: the records of {bad.size} queries differ, first queries {bad[:5]}: {rec[bad[:3]]} "
                           f"({rec[bad[:3], 1:].view(F32)}) for {wrec[bad[:3]]} ({wrec[bad[:3], 1:].view(F32)})")
    assert (rec[live:] == REC_SENTINEL).all(), f"{what}: records past {live} written"
    if points:
        for name, a, b in (("query", qp, wqp), ("scene", pp, wpp)):
            badp = np.flatnonzero((a[:live].view(np.int32) != b[:live].view(np.int32)).any(axis=1))
            assert badp.size == 0, f"{what}: the {name} points of {badp.size} queries differ, first {badp[:5]}: {a[badp[:3]]} for {b[badp[:3]]}"
            assert (a[live:] == PT_SENTINEL).all(), f"{what}: {name} points past {live} written"
    else:
        assert (qp == PT_SENTINEL).all() and (pp == PT_SENTINEL).all(), f"{what}: points written that were not asked for"


def _check_within(w, want, live, what=""):
    assert np.array_equal(w[:live], want[3][:live]), f"{what}: verdicts differ at {np.flatnonzero(w[:live] != want[3][:live])[:5]}"
    assert (w[live:] == W_SENTINEL).all(), f"{what}: verdicts past {live} written"


def _all(sc, case, what, strides=STRIDES, counted=True):
    n = case.n
    for stride in strides:
        w = f"{case.name}, {what}, stride {stride}"
        _check(_distance(sc, case, stride), case.want(False), n, w)
        _check(_distance(sc, case, stride, radii=True), case.want(True), n, w + ", radii")
        _check_within(_within(sc, case, stride), case.want(True), n, w + ", radii")
        if counted:
            cnt = torch.tensor([n - 7], dtype=torch.int32, device=DEV)
            _check(_distance(sc, case, stride, radii=True, count=cnt, points=False), case.want(True), n - 7, w + ", d_count", points=False)
            _check_within(_within(sc, case, stride, radii=False, count=cnt), case.want(False), n - 7, w + ", d_count, no radii")


def _expectation_is_worth_using(case):
    """The conditions on the expectation, before it is used."""
    rec, _, _, _, eligible, D2 = case.want(False)
    dist, hit = rec[:, 1].view(F32), rec[:, 0] >= 0
    assert (hit & (dist == 0)).sum() >= 300
    assert (hit & (dist > 0) & np.isfinite(dist)).sum() >= 300
    rec_r = case.want(True)[0]
    assert (hit & (rec_r[:, 0] < 0)).sum() >= 50 and (hit & (dist > 0) & (rec_r[:, 0] >= 0)).sum() >= 50
    key = np.where(eligible, D2, np.inf)
    low = key.min(axis=1)
    ties = ((key == low[:, None]) & eligible).sum(axis=1)
    assert ((ties >= 2) & (low == 0)).sum() >= 20               # several overlapping candidates, all at 0
    assert ((ties >= 2) & (low > 0) & np.isfinite(low)).sum() >= 20   # a shared vertex or edge nearest
    assert (~hit).sum() >= 10                                   # the non-finite and the zero-area queries


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cube", "blob", "nested", "open", "degenerate", "sliver"])
def test_meshes_against_the_restatement(which, gpu_available):
    case = _case(which)
    _expectation_is_worth_using(case)
    n = case.n
    with case.create() as sc:                                   # freshly created: no update has made the device vertices yet
        sc.bvh_validate()
        assert which != "sliver" or sc.bvh_info()["always"] >= 1
        _all(sc, case, "sah, width 4, fresh")
        for live in Q.PREFIXES:
            cnt = torch.tensor([live], dtype=torch.int32, device=DEV)
            _check(_distance(sc, case, 3, count=cnt), case.want(False), live, f"{which}, d_count {live}")
            _check_within(_within(sc, case, 4, count=cnt), case.want(True), live, f"{which}, d_count {live}")
        sc.tune("bvh_width", 2)
        _all(sc, case, "sah, width 2")
        sc.tune("bvh_width", 4)
        sc.tune("lds_stack", 1)                                 # every push beyond the first through the overflow path
        _all(sc, case, "sah, lds_stack 1", strides=(3,), counted=False)
        sc.tune("lds_stack", 16)
        sc.set_accel("brute_force")
        _all(sc, case, "brute force")
        sc.set_accel("bvh")
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(case.V, "rebuild") in ("rebuilt_lbvh", "rebuilt_" + builder)   # (a tiny mesh may hand over)
            sc.bvh_validate()
            for width in (4, 2):
                sc.tune("bvh_width", width)
                _all(sc, case, f"{builder}, width {width}", strides=(3,) if width == 4 else (4,), counted=False)
        sc.set_profiling(True, count_work=True)                 # the counting instantiations
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _all(sc, case, f"cluster, width {width}, counting", strides=(4,) if width == 4 else (3,), counted=False)
        sc.set_profiling(False)
        # without the optional arrays, through the C entry: the records alone
        rec = torch.full((n + 8, 4), REC_SENTINEL, dtype=torch.int32, device=DEV)
        qt = _dev_tris(case.q, 3, 0)
        rc = _capi.lib().rt_triangle_distance_device(sc.handle, C.c_void_p(qt.data_ptr()), 3, n, None, None, None, 0,
                                                     C.c_void_p(rec.data_ptr()), None, None, None)
        assert rc == _capi.RT_OK
        torch.cuda.synchronize()
        assert np.array_equal(_np(rec)[:n], case.want(False)[0]) and (_np(rec)[n:] == REC_SENTINEL).all()
    # a scene whose first trees are the device builder's, queried before anything else
    with case.create(builder="lbvh") as sc:
        _all(sc, case, "created with lbvh, fresh", strides=(4,), counted=False)


# 2 -------------------------------------------------------------------------------------------------
def test_after_updates_and_mesh_changes(blob):
    """After update_vertices (a refit, from a host array and from a device tensor) and after set_mesh the answers are
    a freshly created scene's."""
    queries = blob.q[::4]
    v1 = (blob.V * F32(1.1)).astype(F32)
    v2 = (blob.V * F32(0.8) + F32(0.05)).astype(F32)
    c0, c1, c2 = Case("blob", blob.V, blob.tri, queries), Case("blob x 1.1", v1, blob.tri, queries), Case("blob moved", v2, blob.tri, queries)
    Vn, trin = DR.MESHES["nested"]()
    on_nested = Case("nested, the blob's queries", Vn, trin, queries)
    nothing = Case("no triangles", np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), queries)
    assert not np.array_equal(c1.want(False)[0], c0.want(False)[0]) and not np.array_equal(c2.want(False)[0], c0.want(False)[0])
    assert (nothing.want(False)[0] == DR.MISS).all()

    def both(sc, case, what):
        _all(sc, case, what, strides=(3,), counted=False)

    with c0.create() as sc:
        both(sc, c0, "fresh")
        assert sc.update_vertices(v1) == "refit"
        for width in (4, 2):
            sc.tune("bvh_width", width)
            both(sc, c1, f"after the host update, width {width}")
        with c1.create() as fresh:                              # ... and a freshly created scene gives the same bytes
            assert np.array_equal(_distance(fresh, c1)[0], _distance(sc, c1)[0])
        assert sc.update_vertices(torch.from_numpy(v2).to(DEV)) == "refit"
        for width in (4, 2):
            sc.tune("bvh_width", width)
            both(sc, c2, f"after the device update, width {width}")
        sc.set_accel("brute_force")
        both(sc, c2, "after the device update, brute force")
        sc.set_accel("bvh")
        for builder in BUILDERS:
            sc.set_builder(builder)
            sc.set_mesh(torch.from_numpy(on_nested.V).to(DEV), torch.from_numpy(on_nested.tri.view(np.int32)).to(DEV),
                        torch.zeros(len(on_nested.tri), dtype=torch.int32, device=DEV))
            for width in (4, 2):
                sc.tune("bvh_width", width)
                both(sc, on_nested, f"after set_mesh ({builder}), width {width}")
            sc.set_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32))
            for accel in ("bvh", "brute_force"):
                sc.set_accel(accel)
                both(sc, nothing, f"no triangles ({builder}, {accel})")
            sc.set_accel("bvh")
            sc.set_mesh(c0.V, c0.tri, np.zeros(len(c0.tri), np.uint32))
            both(sc, c0, f"the blob again ({builder})")


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["blob", "open"])
def test_the_mesh_against_itself(which, gpu_available):
    """self_index = arange on the mesh's own triangles: the triangle and its neighbours are passed over, and the
    answer is the nearest triangle that shares no vertex index with it."""
    V, tri = DR.MESHES[which]()
    own = np.ascontiguousarray(V, F32)[np.asarray(tri, np.int64)]
    n = len(own)
    plain = Case(f"{which}, its own triangles", V, tri, own)
    case = Case(f"{which}, its own triangles, self", V, tri, own, np.arange(n))
    junk = Case(f"{which}, its own triangles, self out of range", V, tri, own, np.where(np.arange(n) % 2 == 0, -1, n + 5))
    rec, rec_self = plain.want(False)[0], case.want(False)[0]
    valid = rec[:, 0] >= 0
    assert valid.sum() >= n - 16 and (rec[valid, 1].view(F32) == 0).all()           # every triangle meets itself or an earlier neighbour
    skip = DR.self_matrix(case.tri, case.self_index, n)
    assert not skip[np.flatnonzero(valid), rec_self[valid, 0]].any()
    assert (rec_self[valid, 0] != rec[valid, 0]).sum() >= 1 and (rec_self[valid, 1].view(F32) > 0).sum() >= n // 2
    assert np.array_equal(junk.want(False)[0], rec)
    with case.create() as sc:
        for accel, width in (("bvh", 4), ("bvh", 2), ("brute_force", 4)):
            sc.set_accel(accel)
            sc.tune("bvh_width", width)
            for c in (case, plain, junk):
                _all(sc, c, f"{accel}, width {width}", strides=(3,), counted=False)


# 4 -------------------------------------------------------------------------------------------------
def test_the_walk_culls_and_the_verdict_stops_early(blob):
    """With RT_PROFILE_WORK the triangle evaluations per query of the tree walk are below the loop's over every
    triangle (the number of triangles), and the verdict's are at most the record's."""
    case = blob
    n, nt = case.n, len(case.tri)
    with case.create() as sc:
        sc.set_profiling(True, count_work=True)
        for builder in BUILDERS:
            sc.set_builder(builder)
            sc.update_vertices(case.V, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                for radii in (False, True):
                    sc.reset_stats()
                    _check(_distance(sc, case, radii=radii), case.want(radii), n, f"{builder}, width {width}")
                    rec_tests, rec_visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                    sc.reset_stats()
                    _check_within(_within(sc, case, radii=radii), case.want(radii), n, f"{builder}, width {width}")
                    any_tests, any_visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                    print(f"{builder}, width {width}, radii {radii}: the record {rec_tests / n:.2f} triangles and {rec_visits / n:.2f} nodes "
                          f"per query, the verdict {any_tests / n:.2f} and {any_visits / n:.2f}; every triangle: {nt}")
                    assert 0 < rec_tests < n * nt and 0 < any_tests <= rec_tests and 0 < any_visits <= rec_visits
        sc.set_profiling(False)


# 5 -------------------------------------------------------------------------------------------------
STREAM_ENTRIES = [
    ("triangle_distance", lambda sc, q, st: sc.triangle_distance(q["tri"], want_points=True, stream=st)),
    ("triangle_distance with radii", lambda sc, q, st: sc.triangle_distance(q["tri"], rmax=q["rmax"], stream=st)),
    ("triangle_within", lambda sc, q, st: sc.triangle_within(q["tri"], rmax=q["rmax"], stream=st)),
]


@pytest.mark.parametrize("name,call", STREAM_ENTRIES, ids=[name for name, _ in STREAM_ENTRIES])
def test_entry_runs_on_the_callers_stream_and_sees_the_update(gpu_available, name, call):
    """tests/test_gpu_query_frame.py's check for the two new methods (their names carry no _device suffix, so its list
    does not hold them): the query on stream A, the same on stream B, a refit, the query on A again; the first two
    are the bytes of the call made on the default stream before the update, the third those of the call after it."""
    import test_gpu_query_frame as QF
    V, tri = IR.blob()
    V = np.ascontiguousarray(V, F32)
    V1 = (V * QF.GROW).astype(F32)
    with R.Scene.create(V, tri, np.zeros(len(tri), np.uint32), IR.MATERIALS, device=0) as sc:
        q = QF._queries()
        torch.cuda.synchronize(DEV)
        A, B = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
        before = QF._bytes(call(sc, q, None))
        with torch.cuda.stream(A):
            on_a = call(sc, q, A)
        with torch.cuda.stream(B):
            on_b = call(sc, q, B)
        assert sc.update_vertices(V1) == "refit"
        with torch.cuda.stream(A):
            on_a_after = call(sc, q, A)
        A.synchronize()
        B.synchronize()
        after = QF._bytes(call(sc, q, None))
        assert before != after, f"{name}: the update changes no answer, so the test would pass without it"
        assert QF._bytes(on_a) == before, f"{name}: stream A before the update"
        assert QF._bytes(on_b) == before, f"{name}: stream B before the update"
        assert QF._bytes(on_a_after) == after, f"{name}: stream A after the update"


# the argument errors on a device scene, each the only thing wrong (tests/test_triangle_distance_capi.py has the order)
def test_argument_errors_on_a_device_scene(blob):
    import test_triangle_distance_capi as TC
    with blob.create() as sc:
        for what, kw in TC.DISTANCE_CASES.items():
            assert TC._distance(sc, **kw) == _capi.RT_E_ARG, what
        for what, kw in TC.SHARED_CASES.items():
            assert TC._within(sc, **kw) == _capi.RT_E_ARG, what
        assert TC._distance(sc, n=0, tris=None, out=None) == _capi.RT_OK and TC._within(sc, n=0, tris=None, out=None) == _capi.RT_OK
        t = torch.zeros((4, 3, 3), dtype=torch.float32, device=DEV)
        for bad in (torch.zeros(3, dtype=torch.float32, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV), np.zeros(4, F32)):
            with pytest.raises(ValueError):
                sc.triangle_distance(t, rmax=bad)
            with pytest.raises(ValueError):
                sc.triangle_within(t, self_index=bad)
