"""tests/_closest_point_ref.py, the numpy restatement of the closest-point definition (include/raytracert.h),
checked on the CPU: against an independent float64 distance from point to triangle, and for the counts that
say no case of tests/test_gpu_closest_point.py passes empty (every region wins, ties occur, misses occur).
"""
import numpy as np
import pytest

import oracle as O
from raytracert_amd import scenes

import _closest_point_ref as CP
import _query_scenes as QS
import _range_ref as RR

F32 = np.float32
EPS = 2.0 ** -24


def _file_triangles(path):
    return RR.scene_triangles(O.OracleScene(path))[0]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("closest_point_ref"))
    out = {}
    Tq = _file_triangles(scenes.write_sphere_grid(QS.SPEC_Q, d, "cp_q"))
    out["q"] = (Tq, CP.points_for(Tq, 101, surface=CP.q_surface_points(Tq)))
    Ts = _file_triangles(CP.write_obj(d, "cp_shingles", CP.shingles_triangles()))
    assert np.array_equal(Ts, CP.shingles_triangles())
    out["shingles"] = (Ts, CP.points_for(Ts, 102))
    Tf = _file_triangles(CP.write_obj(d, "cp_far", CP.far_tiny_triangles()))
    assert np.array_equal(Tf, CP.far_tiny_triangles())      # the file holds the float32 values exactly
    out["far_tiny"] = (Tf, CP.points_for(Tf, 103))
    out["one"] = (CP.one_triangle(), CP.points_for(CP.one_triangle(), 104))
    return {k: (T, p, CP.pairs(p, T)) for k, (T, p) in out.items()}


@pytest.mark.parametrize("which", ["q", "shingles", "far_tiny", "one"])
def test_restatement_against_float64_distance(which, cases):
    """|sqrt(dist2) - true distance| <= 16 * 2^-24 * (m1 + |p|_1) for every finite pair: the rounding of c, r and
    the sum, with m1 the scene's largest |x| + |y| + |z|."""
    T, p, P = cases[which]
    finite = np.isfinite(p).all(axis=1) & (np.abs(p).max(axis=1) < 1e18)
    cand = P["candidate"][0]
    assert finite.sum() >= 200 and cand.all()
    true = CP.true_distance(p[finite], T)
    got = np.sqrt(P["dist2"][finite].astype(np.float64))
    tol = 16 * EPS * (CP.scene_m1(T) + np.abs(p[finite].astype(np.float64)).sum(axis=1))[:, None]
    err = np.abs(got - true)
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"{which}: worst error / bound = {(err / tol).max():.4f} at point {worst[0]}, triangle {worst[1]}")
    assert (err <= tol).all(), f"{which}: error {err[worst]} above {tol[worst[0], 0]} (region {CP.REGIONS[P['region'][finite][worst]]})"
    # s, t stay in the triangle in every region
    s, t = P["s"][finite], P["t"][finite]
    assert (s >= 0).all() and (t >= 0).all() and (s <= 1).all() and ((s.astype(np.float64) + t) <= 1 + EPS).all()


@pytest.mark.parametrize("which", ["q", "shingles", "far_tiny", "one"])
def test_every_region_wins(which, cases):
    T, p, P = cases[which]
    res = CP.closest(P)
    hit = res["triangle"] >= 0
    counts = np.bincount(res["region"][hit], minlength=7)
    print(f"{which}: {len(p)} points, {hit.sum()} answers, winners per region {dict(zip(CP.REGIONS, counts))}, ties {res['ties'].sum()}")
    assert 240 <= len(p) <= 280
    assert (counts >= 1).all(), f"{which}: a region never wins: {dict(zip(CP.REGIONS, counts))}"
    # the non-finite points and those at 1e30 miss; everything else has an answer
    bad = ~np.isfinite(p).all(axis=1) | (np.abs(p).max(axis=1) > 1e29)
    assert bad.sum() == 11 and not hit[bad].any() and hit[~bad].all()
    assert (res["record"][~hit] == np.array([0xFFFFFFFF, CP.INF_BITS, 0, 0], np.uint32)).all()
    assert (res["point"][~hit] == 0).all()


@pytest.mark.parametrize("which", ["q", "far_tiny"])
def test_ties_between_triangles_occur(which, cases):
    """Shared vertices and edges (Q) and lattice vertices (far tiny) give equal dist2 on different triangles; the
    lowest index wins."""
    T, p, P = cases[which]
    res = CP.closest(P)
    assert res["ties"].sum() >= {"q": 8, "far_tiny": 3}[which]
    for i in np.flatnonzero(res["ties"])[:8]:
        d2 = P["dist2"][i, res["triangle"][i]]
        same = np.flatnonzero(P["candidate"][0] & (P["dist2"][i] == d2))
        assert len(same) >= 2 and same[0] == res["triangle"][i]


def test_radius_rule(cases):
    T, p, P = cases["q"]
    full = CP.closest(P)
    dist = full["distance"]
    hit = full["triangle"] >= 0
    up = np.nextafter(dist, F32(np.inf)).astype(F32)
    twice = CP.closest(P, (F32(2) * dist).astype(F32))
    pos = hit & (dist > 0)                 # (a point on the mesh has distance 0: twice that is an empty search)
    assert pos.sum() >= 200 and (hit & ~pos).sum() >= 8
    assert np.array_equal(twice["record"][pos], full["record"][pos]) and (twice["triangle"][hit & ~pos] == -1).all()
    half = CP.closest(P, (F32(0.5) * dist).astype(F32))
    assert (half["triangle"][hit & (dist > 0)] == -1).all()
    at, above = CP.closest(P, dist), CP.closest(P, up)
    # rmax * rmax against dist2: both sides of the rounding occur at rmax = dist, and just above it nearly all are in
    d2 = P["dist2"][np.arange(len(p)), np.maximum(full["triangle"], 0)]
    with np.errstate(all="ignore"):
        inside = hit & (d2 < dist * dist)
    assert np.array_equal(at["triangle"][hit] >= 0, inside[hit])
    assert 20 <= inside.sum() <= hit.sum() - 20
    assert (above["triangle"][hit] >= 0).sum() > inside.sum()
    for r in (0.0, -1.0, np.nan):
        assert (CP.closest(P, np.full(len(p), r, F32))["triangle"] == -1).all()
    assert np.array_equal(CP.closest(P, np.full(len(p), np.inf, F32))["record"], full["record"])


def test_degenerate_and_empty():
    T = CP.degenerate_triangles()
    p = CP.points_for(T, 105)
    P = CP.pairs(p, T)
    assert not P["candidate"].any()
    assert (CP.closest(P)["triangle"] == -1).all()
    assert (CP.closest(CP.pairs(p, np.zeros((0, 3, 3), F32)))["triangle"] == -1).all()
