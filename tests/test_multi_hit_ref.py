"""tests/_multi_hit_ref.py on the CPU: what the expectation of rt_multi_hit_range_device says, built from
tests/_range_ref.py alone (which tests/test_range_ref.py pins to the oracle). first_k(k = 1) is the ranged
closest record; the full list is _range_ref.sorted_hits; the doubled-shingles scene has every distance three
times, lists deeper than three times the largest k, and stepping by nextafter finds one hit of each three.
"""
import numpy as np
import pytest

import oracle as O
from raytracert_amd import _capi, scenes

import _edge_rays as E
import _multi_hit_ref as MH
import _query_scenes as QS
import _range_ref as RR

F32 = np.float32
INF = F32(np.inf)
KMAX = _capi.MULTI_HIT_MAX


class Case:
    def __init__(self, path, o, d):
        self.o, self.d = o, d
        self.T, self.transparent = RR.scene_triangles(O.OracleScene(path))
        self.P = RR.pairs(o, d, self.T)
        for a in self.P.values():
            a.setflags(write=False)
        self.len = RR.ray_length(o, d)
        self.d1, self.d2, self.d3 = (RR.nth_distance(self.P, k) for k in range(3))

    def menu(self):
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
def q(workdir):
    return Case(scenes.write_sphere_grid(QS.SPEC_Q, workdir, "multi_ref_q"), *QS.r200())


@pytest.fixture(scope="module")
def shingles(workdir):
    return Case(E.write_scene(workdir, "multi_ref_shingles"), *E.generic())


@pytest.fixture(scope="module")
def doubled(workdir):
    return Case(MH.write_doubled(workdir, "multi_ref_doubled"), *E.generic())


@pytest.mark.parametrize("which", ["q", "shingles", "doubled"])
def test_first_one_is_the_ranged_closest_record(which, request):
    case = request.getfixturevalue(which)
    for name, kw in case.menu().items():
        b = RR.bounds(case.o, case.d, **kw)
        rec, nhits = MH.first_k(case.P, *b, 1)
        want = RR.closest(case.P, *b)
        assert rec.shape == (len(case.o), 1, 4) and np.array_equal(rec[:, 0], want["record"]), name
        assert np.array_equal(nhits, (want["triangle"] >= 0).astype(np.int32)), name


@pytest.mark.parametrize("which", ["q", "shingles"])
def test_the_list_is_sorted_hits(which, request):
    """The half-line: the rows of first_k(KMAX), then the further rows of a longer list, are sorted_hits."""
    case = request.getfixturevalue(which)
    b = RR.bounds(case.o, case.d)
    m = MH.totals(case.P, *b)
    deep = int(m.max())
    rec, nhits = MH.first_k(case.P, *b, KMAX)
    full, nfull = MH.first_k(case.P, *b, max(deep, KMAX) + 2)
    assert np.array_equal(full[:, :KMAX], rec) and np.array_equal(nhits, np.minimum(m, KMAX)) and np.array_equal(nfull, m)
    for i in range(len(case.o)):
        want = RR.sorted_hits(case.P, i)
        got = [(float(r[1:2].view(F32)[0]), int(r[0])) for r in full[i, :m[i]]]
        assert got == want and len(want) == m[i], i
        assert (full[i, m[i]:] == MH.MISS).all()
        j = np.array([t for _, t in want], np.int64)
        assert np.array_equal(full[i, :m[i], 2], case.P["s"][i, j].view(np.uint32))
        assert np.array_equal(full[i, :m[i], 3], case.P["t"][i, j].view(np.uint32))
    if which == "shingles":
        assert deep == 36 and (m == 0).sum() >= 20


def test_doubled_shingles_come_in_runs_of_three(doubled, shingles):
    b = RR.bounds(doubled.o, doubled.d)
    m = MH.totals(doubled.P, *b)
    assert len(doubled.T) == MH.COPIES * E.N_TRI and np.array_equal(doubled.T[:E.N_TRI], doubled.T[E.N_TRI:2 * E.N_TRI])
    assert np.array_equal(m, MH.COPIES * MH.totals(shingles.P, *RR.bounds(shingles.o, shingles.d)))
    assert m.max() == 108 and (m >= MH.COPIES * KMAX).sum() >= 1        # truncation inside a deep list
    full, _ = MH.first_k(doubled.P, *b, int(m.max()))
    for i in range(len(doubled.o)):
        rows = full[i, :m[i]]
        tri, dist = rows[:, 0].astype(np.int64).reshape(-1, 3), rows[:, 1].reshape(-1, 3)
        assert (dist[:, 0] == dist[:, 1]).all() and (dist[:, 1] == dist[:, 2]).all()
        assert (tri[:, 1] == tri[:, 0] + E.N_TRI).all() and (tri[:, 2] == tri[:, 1] + E.N_TRI).all()     # ascending indices
        assert (np.diff(dist[:, 0].view(F32)) > 0).all()                 # distinct distances between the runs
    # k = 2 and k = 4 cut inside a run and keep the lowest indices
    for k in (1, 2, 4):
        rec, nhits = MH.first_k(doubled.P, *b, k)
        assert np.array_equal(rec, full[:, :k]) and np.array_equal(nhits, np.minimum(m, k))
        assert (rec[:, 0, 0][m > 0] < E.N_TRI).all()


def test_stepping_by_nextafter_finds_a_third_of_the_hits(doubled):
    """The defect the multi-hit query removes: tmin = nextafter(previous distance) passes over the two other
    copies at that distance."""
    n = len(doubled.o)
    m = MH.totals(doubled.P, *RR.bounds(doubled.o, doubled.d))
    found = np.zeros(n, np.int64)
    tmin = np.zeros(n, F32)
    for launch in range(40):
        want = RR.closest(doubled.P, *RR.bounds(doubled.o, doubled.d, tmin=tmin))
        hit = want["triangle"] >= 0
        if not hit.any():
            break
        assert (want["triangle"][hit] < E.N_TRI).all()                  # always the lowest copy
        found += hit
        tmin = np.where(hit, np.nextafter(want["distance"], INF), INF).astype(F32)
    assert launch == 36 and m.sum() > 0 and np.array_equal(MH.COPIES * found, m)
