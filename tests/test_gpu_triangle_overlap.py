"""Triangle-overlap queries (rt_triangle_overlap_device, rt_triangle_collides_device: k_bvh_tri, k_tri): per query
triangle the k lowest indices above `after` of the candidate triangles that meet it and that `self` does not pass
over, their number, and whether there is one; queries and results in torch CUDA tensors.

The expectation is tests/_triangle_overlap_ref.py, the numpy restatement of the definition in include/raytracert.h,
which tests/test_triangle_overlap_ref.py checks on the CPU against an exact integer test. Equality is of bytes
throughout: there is no tolerance. Outputs are filled with sentinels first, so rows past the live count and outputs
that were not asked for are shown to be untouched. The meshes are tests/_box_overlap_ref.py's (cube, blob, nested, open,
degenerate, and the blob with a sliver on the always list); the queries of a mesh are
_triangle_overlap_ref.mesh_queries: 1,024 random triangles of several sizes, the triangle that cuts the whole mesh,
copies of scene triangles and copies shifted in their plane, triangles sharing a vertex or an edge with the scene,
non-finite and zero-area queries, and triangles outside the scene.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import raytracert_amd as R
from raytracert_amd import _capi

import _inside_ref as IR
import _query_scenes as Q
import _triangle_overlap_ref as TR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
TRI_SENTINEL = -7
NF_SENTINEL = -9
COL_SENTINEL = 0xAB
STRIDES = (3, 4)
KS = (1, 4, 16)
BUILDERS = ("sah", "lbvh", "cluster")
INT32_MIN = np.iinfo(np.int32).min


def _np(t):
    return t.cpu().numpy()


def _dev_tris(q, stride, junk):
    """Query triangles as a CUDA tensor in either layout; the padded layout's w holds values that must not matter."""
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    if stride == 4:
        w = np.where(np.arange(3 * len(q)) % 2 == 0, np.nan, junk).astype(F32).reshape(-1, 3, 1)
        q = np.concatenate([q, w], axis=2)
    return torch.from_numpy(np.ascontiguousarray(q)).to(DEV)


def _dev_i32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


class Case:
    """A mesh, its queries, an optional self index per query and the restatement's overlap matrix (with the self
    filter applied), computed once and never changed."""

    def __init__(self, name, V=None, tri=None, queries=None, self_index=None):
        self.name = name
        if V is None:
            V, tri = TR.MESHES[name]()
        self.V, self.tri = np.ascontiguousarray(V, F32), np.ascontiguousarray(tri, np.uint32)
        self.q = TR.mesh_queries(self.V, self.tri) if queries is None else np.ascontiguousarray(queries, F32)
        self.n = len(self.q)
        self.self_index = None if self_index is None else np.ascontiguousarray(self_index, np.int32)
        self._M = None
        self._want = {}

    @property
    def M(self):
        if self._M is None:
            self._M = TR.overlap_matrix(self.q, self.V, self.tri) & ~TR.self_matrix(self.tri, self.self_index, self.n)
            self._M.setflags(write=False)
        return self._M

    def want(self, k, after=None):
        """(tris [n, k], min(m, k) [n], m [n]); `after` None or a key of self.afters."""
        if (k, after) not in self._want:
            res = TR.lists(self.M, k, None if after is None else self.afters[after])
            for a in res:
                a.setflags(write=False)
            self._want[(k, after)] = res
        return self._want[(k, after)]

    @property
    def afters(self):
        rng = np.random.default_rng(80)
        return {"mixed": rng.integers(-3, max(len(self.tri), 1) + 2, self.n).astype(np.int32), "own": np.arange(self.n, dtype=np.int32)}

    def collides(self):
        return (self.M.any(axis=1)).astype(np.uint8)

    def create(self, builder="sah"):
        return R.Scene.create(self.V, self.tri, np.zeros(len(self.tri), np.uint32), TR.MATERIALS, device=0, builder=builder)


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


def _query(sc, case, k, stride=3, count=None, n=None, after=None, count_all=False, stream=None):
    """One list query into sentinel-filled outputs: (tris [cap, k] int32, nfound [cap] int32)."""
    n = case.n if n is None else n
    cap = case.n + 8
    tris = torch.full((cap, k), TRI_SENTINEL, dtype=torch.int32, device=DEV)
    nf = torch.full((cap,), NF_SENTINEL, dtype=torch.int32, device=DEV)
    aft = None if after is None else _dev_i32(case.afters[after][:n])
    slf = None if case.self_index is None else _dev_i32(case.self_index[:n])
    res = sc.triangle_overlap_device(_dev_tris(case.q[:n], stride, 123.0), k, after=aft, self_index=slf, count=count, count_all=count_all,
                                     out=(tris, nf), stream=stream)
    assert res[0].shape == (n, k) and res[0].dtype == torch.int32 and res[0].data_ptr() == tris.data_ptr()
    assert res[1].shape == (n,) and res[1].dtype == torch.int32 and res[1].data_ptr() == nf.data_ptr()
    return _np(tris), _np(nf)


def _collides(sc, case, stride=3, count=None, n=None, stream=None):
    n = case.n if n is None else n
    col = torch.full((case.n + 8,), COL_SENTINEL, dtype=torch.uint8, device=DEV)
    slf = None if case.self_index is None else _dev_i32(case.self_index[:n])
    res = sc.triangle_collides_device(_dev_tris(case.q[:n], stride, np.inf), self_index=slf, count=count, out=col, stream=stream)
    assert res.shape == (n,) and res.dtype == torch.uint8 and res.data_ptr() == col.data_ptr()
    return _np(col)


def _check(got, want, live, what="", count_all=False):
    tris, nf = got
    wt, wn, wm = want
    bad = np.flatnonzero((tris[:live] != wt[:live]).any(axis=1))
    assert bad.size == 0, f"{what}: the lists of {bad.size} queries differ, first queries {bad[:5]}: {tris[bad[:3]]} for {wt[bad[:3]]}"
    wc = wm if count_all else wn
    badc = np.flatnonzero(nf[:live] != wc[:live])
    assert badc.size == 0, f"{what}: the counts of {badc.size} queries differ, first queries {badc[:5]}: {nf[badc[:5]]} for {wc[badc[:5]]}"
    assert (tris[live:] == TRI_SENTINEL).all() and (nf[live:] == NF_SENTINEL).all(), f"{what}: rows past {live} written"


def _check_collides(col, want, live, what=""):
    assert np.array_equal(col[:live], want[:live]), f"{what}: verdicts differ at {np.flatnonzero(col[:live] != want[:live])[:5]}"
    assert (col[live:] == COL_SENTINEL).all(), f"{what}: verdicts past {live} written"


def _all(sc, case, what, ks=KS, strides=STRIDES, counted=True):
    n = case.n
    for k, stride in itertools.product(ks, strides):
        w = f"{case.name}, {what}, k {k}, stride {stride}"
        _check(_query(sc, case, k, stride), case.want(k), n, w)
        if counted:
            cnt = torch.tensor([n - 7], dtype=torch.int32, device=DEV)
            _check(_query(sc, case, k, stride, count=cnt, count_all=True), case.want(k), n - 7, w + ", d_count", count_all=True)
    for stride in strides:
        _check_collides(_collides(sc, case, stride), case.collides(), n, f"{case.name}, {what}, stride {stride}")


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cube", "blob", "nested", "open", "degenerate", "sliver"])
def test_meshes_against_the_restatement(which, gpu_available):
    case = _case(which)
    assert case.n >= 1024 + 250
    m = case.M.sum(axis=1)
    # the spanning triangle overflows every k (a plane cuts 64 of the blob's 512 triangles at the most, and more of
    # the two meshes that the paging test uses)
    assert m.max() > (16 * 4 if which in ("nested", "degenerate") else 16) or which == "cube"
    assert (m[-10:] == 0).all() and (m == 0).sum() >= 50 and (m > 0).sum() >= 300
    with case.create() as sc:                                   # freshly created: no update has made the device vertices yet
        sc.bvh_validate()
        assert which != "sliver" or sc.bvh_info()["always"] >= 1
        _all(sc, case, "sah, width 4, fresh")
        for live in Q.PREFIXES:
            cnt = torch.tensor([live], dtype=torch.int32, device=DEV)
            _check(_query(sc, case, 4, 3, count=cnt), case.want(4), live, f"{which}, d_count {live}")
            _check_collides(_collides(sc, case, 4, count=cnt), case.collides(), live, f"{which}, d_count {live}")
        sc.tune("bvh_width", 2)
        _all(sc, case, "sah, width 2")
        sc.tune("bvh_width", 4)
        sc.tune("lds_stack", 1)                                 # every push beyond the first through the overflow path
        _all(sc, case, "sah, lds_stack 1", ks=(4,), strides=(3,), counted=False)
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
                _all(sc, case, f"{builder}, width {width}", ks=(1, 16) if width == 4 else (4,))
        sc.set_profiling(True, count_work=True)                 # the counting instantiations
        for width in (4, 2):
            sc.tune("bvh_width", width)
            _all(sc, case, f"cluster, width {width}, counting", ks=(4,))
        sc.set_profiling(False)
    # a scene whose first trees are the device builder's, queried before anything else
    with case.create(builder="lbvh") as sc:
        _all(sc, case, "created with lbvh, fresh", ks=(16,), strides=(4,), counted=False)


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nested", "degenerate"])
def test_count_all_and_paging(which, gpu_available):
    case = _case(which)
    n = case.n
    whole = int(np.argmax(case.M.sum(axis=1)))
    everything = np.flatnonzero(case.M[whole])
    assert len(everything) > 16 * 4
    with case.create() as sc:
        for accel, width in (("bvh", 4), ("bvh", 2), ("brute_force", 4)):
            sc.set_accel(accel)
            sc.tune("bvh_width", width)
            what = f"{which}, {accel}, width {width}"
            for k in KS:
                plain, counted = _query(sc, case, k), _query(sc, case, k, count_all=True)
                _check(plain, case.want(k), n, what)
                _check(counted, case.want(k), n, what + ", count all", count_all=True)
                assert np.array_equal(plain[0], counted[0]), f"{what}: the list depends on the flag"
                assert counted[1][whole] == len(everything) and plain[1][whole] == k
                for count_all in (False, True):
                    _check(_query(sc, case, k, 4, after="mixed", count_all=count_all), case.want(k, "mixed"), n, what + ", after", count_all)
            # paging through the spanning query: every candidate exactly once, in index order
            k, got, last = 16, [], -1
            qt = torch.from_numpy(case.q[whole:whole + 1]).to(DEV)
            for _ in range(len(everything) // k + 2):
                tris, nf = sc.triangle_overlap_device(qt, k, after=torch.tensor([last], dtype=torch.int32, device=DEV), count_all=True)
                tris, left = _np(tris)[0], int(_np(nf)[0])
                assert left == len(everything) - len(got), what
                if left == 0:
                    assert (tris == -1).all()
                    break
                page = tris[:min(left, k)]
                assert (page >= 0).all() and (tris[min(left, k):] == -1).all()
                got += page.tolist()
                last = int(page[-1])
            assert got == everything.tolist(), f"{what}: paging"
        # without d_nfound_out, d_after and d_self, through the C entry: the list alone, and nothing else written
        sc.set_accel("bvh")
        tris = torch.full((n + 8, 4), TRI_SENTINEL, dtype=torch.int32, device=DEV)
        qt = _dev_tris(case.q, 3, 0)
        rc = _capi.lib().rt_triangle_overlap_device(sc.handle, C.c_void_p(qt.data_ptr()), 3, n, None, None, None, 0, 4,
                                                    C.c_void_p(tris.data_ptr()), None, None)
        assert rc == _capi.RT_OK
        torch.cuda.synchronize()
        assert np.array_equal(_np(tris)[:n], case.want(4)[0]) and (_np(tris)[n:] == TRI_SENTINEL).all()


# 3 -------------------------------------------------------------------------------------------------
def test_the_verdict_stops_at_the_first_overlap(blob):
    """rt_triangle_collides_device equals m > 0 (every mesh and tree shape: test 1), and with RT_PROFILE_WORK its
    triangle visits per query stay below the list walk's on the same queries: it leaves a query at its first overlap."""
    case = Case("blob, queries that overlap", blob.V, blob.tri, blob.q[blob.M.any(axis=1)])
    n = case.n
    assert n >= 300
    with case.create() as sc:
        sc.set_profiling(True, count_work=True)
        for builder in BUILDERS:
            sc.set_builder(builder)
            sc.update_vertices(case.V, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                sc.reset_stats()
                _check(_query(sc, case, 16, count_all=True), case.want(16), n, f"{builder}, width {width}", count_all=True)
                list_tests, list_visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                sc.reset_stats()
                _check_collides(_collides(sc, case), np.ones(n, np.uint8), n, f"{builder}, width {width}")
                any_tests, any_visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                print(f"{builder}, width {width}: the verdict {any_tests / n:.2f} triangles and {any_visits / n:.2f} nodes per query, "
                      f"the list {list_tests / n:.2f} and {list_visits / n:.2f}")
                assert 0 < any_tests < list_tests and 0 < any_visits <= list_visits
        sc.set_profiling(False)


# 4 -------------------------------------------------------------------------------------------------
def test_after_updates_and_mesh_changes(blob, nested):
    """Every state the device vertices can be in: a host update, a device update (before and after a first query),
    set_mesh from device tensors, set_mesh to no triangles."""
    queries, n = blob.q, blob.n
    v1 = (blob.V * F32(1.1)).astype(F32)
    v2 = (blob.V * F32(0.8) + F32(0.05)).astype(F32)
    c1, c2 = Case("blob x 1.1", v1, blob.tri, queries), Case("blob moved", v2, blob.tri, queries)
    on_nested = Case("nested, the blob's queries", nested.V, nested.tri, queries)
    nothing = Case("no triangles", np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), queries)
    assert not np.array_equal(c1.want(4)[0], blob.want(4)[0]) and not np.array_equal(c2.want(4)[0], blob.want(4)[0])

    def both(sc, case, what, k=4, stride=3):
        _check(_query(sc, case, k, stride, count_all=True), case.want(k), n, what, count_all=True)
        _check_collides(_collides(sc, case, stride), case.collides(), n, what)

    with blob.create() as sc:
        both(sc, blob, "fresh")
        assert sc.update_vertices(v1) == "refit"                # host array
        for width in (4, 2):
            sc.tune("bvh_width", width)
            both(sc, c1, f"after the host update, width {width}", 16, 4)
        assert sc.update_vertices(torch.from_numpy(v2).to(DEV)) == "refit"
        for width in (4, 2):
            sc.tune("bvh_width", width)
            both(sc, c2, f"after the device update, width {width}")
        sc.set_accel("brute_force")
        both(sc, c2, "after the device update, brute force")
        sc.set_accel("bvh")
        for builder in BUILDERS:
            sc.set_builder(builder)
            v = torch.from_numpy(nested.V).to(DEV)
            t = torch.from_numpy(nested.tri.view(np.int32)).to(DEV)
            m = torch.zeros(len(nested.tri), dtype=torch.int32, device=DEV)
            sc.set_mesh(v, t, m)
            for width in (4, 2):
                sc.tune("bvh_width", width)
                both(sc, on_nested, f"after set_mesh_device ({builder}), width {width}", 16 if width == 4 else 1)
            sc.set_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32))
            for accel in ("bvh", "brute_force"):
                sc.set_accel(accel)
                both(sc, nothing, f"no triangles ({builder}, {accel})", 4, 4)
            sc.set_accel("bvh")
            sc.set_mesh(blob.V, blob.tri, np.zeros(len(blob.tri), np.uint32))      # host arrays: the blob again
            both(sc, blob, f"the blob again ({builder})")
    # the first thing that happens to a fresh scene is a device update; then a rebuild from a host array
    with blob.create() as sc:
        assert sc.update_vertices(torch.from_numpy(v1).to(DEV)) == "refit"
        both(sc, c1, "a device update first")
        assert sc.update_vertices(v2, "rebuild") == "rebuilt"
        both(sc, c2, "then a rebuild")
    # ... and a query first, then the first update: the refit finds its buffers half made and completes them
    with blob.create() as sc:
        both(sc, blob, "a query first")
        assert sc.update_vertices(torch.from_numpy(v2).to(DEV)) == "refit"
        sc.bvh_validate()
        both(sc, c2, "then the first update")


# 5 -------------------------------------------------------------------------------------------------
def test_the_walk_culls(blob):
    """With RT_PROFILE_WORK on the blob, its 1,024 random queries (vertices within 0.3 of the extent of their centre
    at the most): the leaf triangles met per query stay below nt / 4 on every builder and width (a cap, not a
    measurement; the loop over every triangle meets nt), and the bytes are the brute-force accel's. The restatement's
    count of the triangles that survive step 1, which every walk must meet, shows how far inside the cap the inputs
    are."""
    case = Case("blob, random", blob.V, blob.tri, blob.q[:1024])
    n, nt = case.n, len(blob.tri)
    survivors = TR.step1_survivors(case.q, case.V, case.tri).sum() / n
    print(f"step 1 leaves {survivors:.2f} of {nt} triangles per query")
    assert survivors < nt / 16
    with case.create() as sc:
        sc.set_accel("brute_force")
        brute = _query(sc, case, 16, count_all=True)
        brute_col = _collides(sc, case)
        _check(brute, case.want(16), n, "brute force", count_all=True)
        sc.set_accel("bvh")
        sc.set_profiling(True, count_work=True)
        for builder in BUILDERS:
            sc.set_builder(builder)
            sc.update_vertices(blob.V, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                sc.reset_stats()
                got = _query(sc, case, 16, count_all=True)
                tests, visits = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                assert np.array_equal(got[0], brute[0]) and np.array_equal(got[1], brute[1]), f"{builder}, width {width}"
                assert np.array_equal(_collides(sc, case), brute_col)
                print(f"{builder}, width {width}: {tests / n:.2f} triangles, {visits / n:.2f} node visits per query ({nt} triangles)")
                assert 0 < tests / n < nt / 4 and visits > 0, f"{builder}, width {width}: {tests / n:.2f} triangles per query"
        sc.set_profiling(False)


# 6 -------------------------------------------------------------------------------------------------
def test_stream_order_and_updates(blob):
    """Queries queued on two streams before update_vertices answer for the old vertices, those queued after it for
    the new."""
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    reps, n, k = 16, blob.n, 4
    v1 = (blob.V * F32(1.1)).astype(F32)
    moved = Case("blob x 1.1", v1, blob.tri, blob.q)
    old, now = blob.want(k), moved.want(k)
    assert (old[0] != now[0]).any(axis=1).sum() >= 50
    with blob.create() as sc:
        with torch.cuda.stream(s1):
            qt = _dev_tris(blob.q, 3, 0)
            t1, n1 = sc.triangle_overlap_device(qt.repeat(reps, 1, 1), k, count_all=True)      # (the current stream: s1)
        s1.synchronize()                                        # (qt is made; the second stream only reads it)
        with torch.cuda.stream(s2):
            o1 = sc.triangle_collides_device(qt.repeat(reps, 1, 1), stream=s2)
        assert sc.update_vertices(v1) == "refit"
        with torch.cuda.stream(s1):
            t2, n2 = sc.triangle_overlap_device(qt, k, count_all=True, stream=s1)
        with torch.cuda.stream(s2):
            o2 = sc.triangle_collides_device(qt, stream=s2)
        s1.synchronize()
        s2.synchronize()
        assert np.array_equal(_np(t1).reshape(reps, n, k), np.tile(old[0], (reps, 1, 1)))
        assert np.array_equal(_np(n1).reshape(reps, n), np.tile(old[2], (reps, 1)))
        assert np.array_equal(_np(o1).reshape(reps, n), np.tile(blob.collides(), (reps, 1)))
        assert np.array_equal(_np(t2), now[0]) and np.array_equal(_np(n2), now[2])
        assert np.array_equal(_np(o2), moved.collides())


# 7 -------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device_scene(blob):
    """Each RT_E_ARG case alone on a scene with a device; nothing is written."""
    L = _capi.lib()
    qt = _dev_tris(blob.q[:8], 4, 1.0)
    tris = torch.full((16, 4), TRI_SENTINEL, dtype=torch.int32, device=DEV)
    nf = torch.full((16,), NF_SENTINEL, dtype=torch.int32, device=DEV)
    col = torch.full((16,), COL_SENTINEL, dtype=torch.uint8, device=DEV)
    aft = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    slf = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    cnt = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with blob.create() as sc:
        good = dict(q=vp(qt), stride=4, n=8, count=vp(cnt), after=vp(aft), self=vp(slf), flags=0, k=4, out=vp(tris), nf=vp(nf), col=vp(col))

        def overlap(**kw):
            a = dict(good, **kw)
            return L.rt_triangle_overlap_device(sc.handle, a["q"], a["stride"], a["n"], a["count"], a["after"], a["self"], a["flags"], a["k"],
                                                a["out"], a["nf"], None)

        def collides(**kw):
            a = dict(good, **kw)
            return L.rt_triangle_collides_device(sc.handle, a["q"], a["stride"], a["n"], a["count"], a["self"], a["flags"], a["col"], None)

        shared = [dict(n=-1), dict(stride=5), dict(stride=0), dict(q=None), dict(q=vp(qt, 4), n=7), dict(q=vp(qt, 8), n=7),
                  dict(stride=3, q=vp(qt, 2)), dict(stride=3, q=vp(qt, 1)), dict(count=vp(cnt, 2)), dict(self=vp(slf, 2)), dict(flags=1 << 31),
                  dict(flags=_capi.NEAR_COUNT_ALL), dict(flags=_capi.MULTI_COUNT_ALL)]
        for kw in shared + [dict(k=0), dict(k=17), dict(k=-1), dict(out=None), dict(out=vp(tris, 2)), dict(nf=vp(nf, 2)), dict(after=vp(aft, 1)),
                            dict(flags=1), dict(flags=_capi.TRI_COUNT_ALL, nf=None), dict(flags=_capi.TRI_COUNT_ALL | 2),
                            dict(n=(1 << 27) + 1, k=16)]:
            assert overlap(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        for kw in shared + [dict(col=None), dict(flags=1), dict(flags=_capi.TRI_COUNT_ALL)]:
            assert collides(**kw) == _capi.RT_E_ARG, kw
            assert L.rt_last_error_string()
        # in the stated order: the stride before the array, k before the outputs, the flags before n * k
        assert overlap(stride=5, q=None) == _capi.RT_E_ARG and "stride" in L.rt_last_error_string().decode()
        assert overlap(k=0, out=None) == _capi.RT_E_ARG and "k must" in L.rt_last_error_string().decode()
        assert overlap(flags=1, n=(1 << 27) + 1, k=16) == _capi.RT_E_ARG and "flag" in L.rt_last_error_string().decode()
        assert overlap(n=0, q=None, out=None, nf=None) == _capi.RT_OK                      # n == 0: nothing to do
        assert collides(n=0, q=None, col=None) == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(tris) == TRI_SENTINEL).all() and (_np(nf) == NF_SENTINEL).all() and (_np(col) == COL_SENTINEL).all()   # nothing was written
        assert overlap() == _capi.RT_OK and collides() == _capi.RT_OK
        assert overlap(nf=None, after=None, count=None, self=None) == _capi.RT_OK
        torch.cuda.synchronize()
        assert (_np(tris)[:8] != TRI_SENTINEL).all() and (_np(tris)[8:] == TRI_SENTINEL).all()
        assert (_np(nf)[:8] >= 0).all() and (_np(nf)[8:] == NF_SENTINEL).all()
        assert (_np(col)[:8] <= 1).all() and (_np(col)[8:] == COL_SENTINEL).all()
        for kw in (dict(out=tris), dict(out=(tris, nf[:4])), dict(out=(tris[:, :2], nf)), dict(out=(nf, tris)),
                   dict(count=torch.tensor([8], dtype=torch.int64, device=DEV)), dict(after=aft[:4]), dict(after=aft.to(torch.int64)),
                   dict(after=np.zeros(8, np.int32)), dict(self_index=slf[:4]), dict(self_index=slf.to(torch.int64)),
                   dict(self_index=np.zeros(8, np.int32)), dict(self_index=slf.cpu())):
            with pytest.raises(ValueError):
                sc.triangle_overlap_device(qt, 4, **kw)
        for kw in (dict(out=col[:4]), dict(out=nf), dict(count=torch.tensor([8.0], device=DEV)), dict(self_index=slf[:4])):
            with pytest.raises(ValueError):
                sc.triangle_collides_device(qt, **kw)
        with pytest.raises(ValueError):
            sc.triangle_overlap_device(qt.reshape(-1, 4), 4)
        empty = torch.zeros((0, 3, 3), dtype=torch.float32, device=DEV)
        t0, n0 = sc.triangle_overlap_device(empty, 4)
        assert t0.shape == (0, 4) and n0.shape == (0,) and sc.triangle_collides_device(empty).shape == (0,)


# 8 -------------------------------------------------------------------------------------------------
def _own(name, V, tri, self_index="own"):
    """The scene's own triangles as the queries, self_index the query's own index (or the given array, or None)."""
    tri = np.ascontiguousarray(tri, np.uint32)
    q = np.asarray(V, F32)[tri.astype(np.int64)]
    s = np.arange(len(tri), dtype=np.int32) if isinstance(self_index, str) else self_index
    return Case(name, V, tri, q, s)


def test_self_intersection(blob):
    """Query i = scene triangle i with self_index = after = arange lists every intersecting pair of triangles without
    a common vertex index exactly once, at its lower index: on two blobs merged with an offset exactly the restatement's
    pairs (and there are some), on the cube and on a single blob nothing. Without self_index every triangle lists
    itself and its neighbours; a self_index that names no triangle passes nothing over."""
    nv, nt = len(blob.V), len(blob.tri)
    V2 = np.concatenate([blob.V, (blob.V + F32(0.25)).astype(F32)])
    tri2 = np.concatenate([blob.tri, blob.tri + np.uint32(nv)])
    two = _own("two blobs", V2, tri2)
    pairs = np.argwhere(np.triu(two.M))
    assert len(pairs) > 50 and np.array_equal(two.M, two.M.T)
    assert not two.M[:nt, :nt].any() and not two.M[nt:, nt:].any()      # each blob alone does not cut itself
    assert two.M.sum(axis=1).max() <= 16                                # (one call lists every pair)
    cube_v, cube_t = TR.MESHES["cube"]()
    cube, single = _own("cube", cube_v, cube_t), _own("blob", blob.V, blob.tri)
    assert not cube.M.any() and not single.M.any()
    for case in (two, cube, single):
        with case.create() as sc:
            for accel, width in (("bvh", 4), ("bvh", 2), ("brute_force", 4)):
                sc.set_accel(accel)
                sc.tune("bvh_width", width)
                what = f"{case.name}, {accel}, width {width}"
                for stride in STRIDES:
                    got = _query(sc, case, 16, stride, after="own", count_all=True)
                    _check(got, case.want(16, "own"), case.n, what, count_all=True)
                    found = {(i, int(t)) for i in range(case.n) for t in got[0][i] if t >= 0}
                    if case is two:
                        assert found == {(int(i), int(t)) for i, t in pairs}, what
                    else:
                        assert not found and (got[1][:case.n] == 0).all(), what
                # without `after` each pair comes from both sides; the verdict marks the triangles that are cut
                _check(_query(sc, case, 16, count_all=True), case.want(16), case.n, what + ", no after", count_all=True)
                _check_collides(_collides(sc, case), case.collides(), case.n, what)
            sc.set_accel("bvh")
    assert two.collides().sum() == len(set(pairs.ravel().tolist())) > 50
    # without self_index, and with one that names no triangle: itself and every neighbour
    plain = _own("blob, no self", blob.V, blob.tri, None)
    shares = TR.self_matrix(blob.tri, np.arange(nt), nt)
    assert (plain.M & shares).sum() == shares.sum() and (shares.sum(axis=1) >= 10).all()
    with plain.create() as sc:
        _check(_query(sc, plain, 16, count_all=True), plain.want(16), nt, "no self_index", count_all=True)
        _check_collides(_collides(sc, plain), np.ones(nt, np.uint8), nt, "no self_index")
        for value in (-1, nt, INT32_MIN, np.iinfo(np.int32).max):
            case = _own(f"blob, self {value}", blob.V, blob.tri, np.full(nt, value, np.int32))
            assert np.array_equal(case.M, plain.M)
            for width in (4, 2):
                sc.tune("bvh_width", width)
                _check(_query(sc, case, 16, 4, count_all=True), plain.want(16), nt, f"self_index {value}", count_all=True)
                _check_collides(_collides(sc, case, 4), np.ones(nt, np.uint8), nt, f"self_index {value}")
        # a self_index of another triangle than the query's own: that one and its neighbours are passed over
        other = _own("blob, self of the next triangle", blob.V, blob.tri, (np.arange(nt, dtype=np.int32) + 1) % nt)
        assert not np.array_equal(other.M, plain.M) and other.M.any()
        sc.tune("bvh_width", 4)
        _check(_query(sc, other, 16, count_all=True), other.want(16), nt, "self_index of the next triangle", count_all=True)
        _check_collides(_collides(sc, other), other.collides(), nt, "self_index of the next triangle")
