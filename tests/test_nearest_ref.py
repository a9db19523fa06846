"""tests/_nearest_ref.py, the expectation of the nearest-triangle queries, checked on the CPU: its order against an
independent float64 distance, its k = 1 rows against the closest-point restatement, and the counts that say no
case of tests/test_gpu_nearest.py passes empty (lists cut by k, lists shorter than k, ties cut by the list's end).
"""
import numpy as np
import pytest

import oracle as O
from raytracert_amd import scenes

import _closest_point_ref as CP
import _nearest_ref as NR
import _query_scenes as QS
import _range_ref as RR

F32 = np.float32
EPS = 2.0 ** -24
MISS = np.array([0xFFFFFFFF, CP.INF_BITS, 0, 0], np.uint32)


def _file_triangles(path):
    return RR.scene_triangles(O.OracleScene(path))[0]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("nearest_ref"))
    out = {}
    Tq = _file_triangles(scenes.write_sphere_grid(QS.SPEC_Q, d, "cp_q"))
    out["q"] = (Tq, CP.points_for(Tq, 101, surface=CP.q_surface_points(Tq)))
    out["shingles"] = (CP.shingles_triangles(), CP.points_for(CP.shingles_triangles(), 102))
    out["far_tiny"] = (CP.far_tiny_triangles(), CP.points_for(CP.far_tiny_triangles(), 103))
    out["one"] = (CP.one_triangle(), CP.points_for(CP.one_triangle(), 104))
    return {k: (T, p, CP.pairs(p, T)) for k, (T, p) in out.items()}


@pytest.mark.parametrize("which", ["q", "shingles", "far_tiny", "one"])
def test_order_against_float64_distance(which, cases):
    """Wherever the float64 distances of two triangles differ by more than 16 * 2^-24 * (m1 + |p|_1), the rounding
    bound of the closest-point tests, the restatement lists them in the float64 order: along a point's whole list
    no triangle comes after one whose true distance is larger by more than the bound."""
    T, p, P = cases[which]
    finite = np.flatnonzero(np.isfinite(p).all(axis=1) & (np.abs(p).max(axis=1) < 1e18))
    assert len(finite) >= 200
    Pf = {k: (v if k == "candidate" else v[finite]) for k, v in P.items()}
    mask, key, order = NR.admitted(Pf)
    assert mask.all()                                          # every pair is admitted: the list is every triangle
    true = np.take_along_axis(CP.true_distance(p[finite], T), order, axis=1)
    tol = 16 * EPS * (CP.scene_m1(T) + np.abs(p[finite].astype(np.float64)).sum(axis=1))[:, None]
    if true.shape[1] > 1:
        before = np.maximum.accumulate(true, axis=1)[:, :-1]   # the largest true distance earlier in the list
        excess = (before - true[:, 1:]) / tol
        print(f"{which}: largest inversion / bound = {excess.max():.4f}")
        assert (excess <= 1).all()
    # ... and the keys themselves ascend, equal ones by index
    sk = np.take_along_axis(key, order, axis=1)
    assert (np.diff(sk, axis=1) >= 0).all()
    same = np.diff(sk, axis=1) == 0
    assert (np.diff(order, axis=1)[same] > 0).all()


@pytest.mark.parametrize("which", ["q", "shingles", "far_tiny", "one"])
def test_k1_rows_are_the_closest_point(which, cases):
    T, p, P = cases[which]
    n = len(p)
    base = CP.closest(P)["distance"]
    for rmax in (None, np.full(n, 0.05, F32), (F32(2) * base).astype(F32), base,
                 np.where(np.arange(n) % 2 == 0, F32(np.nan), F32(-1)).astype(F32)):
        want = CP.closest(P, rmax)
        got = NR.nearest(P, 1, rmax)
        assert np.array_equal(got["record"][:, 0], want["record"])
        assert np.array_equal(got["point"][:, 0].view(np.uint32), want["point"].view(np.uint32))
        assert np.array_equal(got["within"], (want["triangle"] >= 0).astype(np.uint8))
        assert np.array_equal(got["within"], NR.within(P, rmax))
        assert np.array_equal(got["nfound"], (want["triangle"] >= 0).astype(np.int32))
    # longer lists start with the shorter ones, and miss rows follow the list
    r16 = NR.nearest(P, min(16, NR.K_MAX), np.full(n, 0.05, F32))
    for k in NR.KS:
        rk = NR.nearest(P, k, np.full(n, 0.05, F32))
        assert np.array_equal(rk["record"], r16["record"][:, :k]) and np.array_equal(rk["m"], r16["m"])
        rows = np.arange(k)[None, :] >= rk["nfound"][:, None]
        assert (rk["record"][rows] == MISS).all() and (rk["point"][rows] == 0).all()
        assert (rk["triangle"][~rows] >= 0).all()


def test_counts_on_scene_q(cases):
    """Scene Q's point set with rmax = 0.05 everywhere: for every k lists cut by k, lists shorter than k, and ties cut
    by the list's end (equal dist2 at places k and k + 1)."""
    T, p, P = cases["q"]
    n = len(p)
    assert n == 272 and (CP.closest(P)["triangle"] >= 0).sum() == 261
    rmax = np.full(n, 0.05, F32)
    for k in NR.KS:
        r = NR.nearest(P, k, rmax)
        cut, partial, ties = (r["m"] > k).sum(), ((r["m"] > 0) & (r["m"] < k)).sum(), r["cut_tie"].sum()
        print(f"k {k}: {cut} lists cut, {partial} partial, {ties} ties at the cut, {(r['m'] == 0).sum()} empty")
        assert cut >= 50
        if k >= 2:
            assert partial >= 10
        assert ties >= 10


@pytest.mark.parametrize("which", ["shingles", "far_tiny"])
def test_counts_at_twice_the_closest_distance(which, cases):
    T, p, P = cases[which]
    r = NR.nearest(P, 4, NR.twice_closest(P))
    cut, partial = (r["m"] > 4).sum(), ((r["m"] > 0) & (r["m"] < 4)).sum()
    print(f"{which}: {cut} lists cut, {partial} partial")
    assert cut >= 50 and partial >= 50


def test_degenerate_and_empty():
    T = CP.degenerate_triangles()
    p = CP.points_for(T, 105)
    for TT in (T, np.zeros((0, 3, 3), F32)):
        r = NR.nearest(CP.pairs(p, TT), 4)
        assert (r["record"] == MISS).all() and (r["point"] == 0).all() and (r["nfound"] == 0).all() and (r["m"] == 0).all()
        assert (r["within"] == 0).all()
