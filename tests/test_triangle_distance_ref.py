"""The triangle-distance expectation (tests/_triangle_distance_ref.py, the numpy restatement of include/raytracert.h)
against an exact rational distance of the two closed triangles, on the CPU.

The exact distance is 0 where _triangle_overlap_ref.exact_overlap holds and else the minimum over the same fifteen
feature pairs by exact projection (integers and fractions.Fraction). The pairs are the overlap tests' lattice sets
(generic, coplanar, touching: coordinates multiples of 1/16 within +-3, where the overlap verdict is exact), generic
binary32 pairs around the origin and far from it, and pairs with parallel and collinear edges. On every pair that does
not overlap |sqrt(dist2) - d| <= c * 2^-53 * M with c = 37, the proof's constant as include/raytracert.h states it
(DESIGN.md §7 "Triangle-distance queries" derives 36.5 for the side the cull needs; the other side, a computed distance above the
true one, has no general bound: it is the conditioning of the parameters' quotients and holds on these sets), and
M = max_j |V_j|_1 + 2 max_j |Q_j|_1 of the pair. No pair is left out of any set.

Only test_the_header_states_what_is_restated depends on the entries themselves: the other tests compare the
restatement with the exact checkers and need no library, so they would pass before the entries existed. They are the
ground under tests/test_gpu_triangle_distance.py, which compares the entries' bytes with the restatement, and under
tests/test_triangle_distance_capi.py; those call the entries.
"""
import math
from fractions import Fraction

import numpy as np

import _inside_ref as IR
import _triangle_distance_ref as DR
import _triangle_overlap_ref as TR

F32 = np.float32
F64 = np.float64
EPS = 2.0 ** -53


def test_the_header_states_what_is_restated():
    """The restatement follows include/raytracert.h: the entry's comment must carry the definition's operations."""
    import re

    from raytracert_amd import _capi
    text = open(_capi.HEADER_PATH).read()
    start = text.index("The scene triangle nearest to each query triangle")
    doc = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("int rt_triangle_distance_device(", start)])
    for phrase in ("NaN or infinite component, or n_Q exactly (0,0,0)", "segments and points as degenerate queries are out of scope",
                   "record normal is not (0,0,0)", "index compares, no geometry", "V_j = xyz[tri_v[3 t + j]]", "not the records",
                   "binary64 without contraction", "u_j[a] = (double)Q_j[a] - (double)Q_0[a]", "v_j[a] = (double)V_j[a] - (double)Q_0[a]",
                   "dot(x, y) = (x[0] y[0] + x[1] y[1]) + x[2] y[2]", "if (x < 0) x = 0; if (x > 1) x = 1",
                   "ab = b - a, ac = c - a, w = p - a, d1 = dot(ab, w), d2 = dot(ac, w)",
                   "uu = dot(ab, ab), uv = dot(ab, ac), vv = dot(ac, ac)", "the seven cases of rt_closest_point_device",
                   "interior clamp included", "x[k] = (a[k] + s ab[k]) + t ac[k]",
                   "g = p1 - p0, h = r1 - r0, r = p0 - r0, a = dot(g, g), e = dot(h, h), f = dot(h, r), c = dot(g, r), b = dot(g, h), den = a e - b b",
                   "sq = den != 0 ? clamp01((b f - c e) / den) : 0", "a zero denominator: sq = 0", "tv = (b sq + f) / e",
                   "if (tv < 0) { tv = 0; sq = clamp01(-c / a); } else if (tv > 1) { tv = 1; sq = clamp01((b - c) / a); }",
                   "x[k] = p0[k] + sq g[k], y[k] = r0[k] + tv h[k]", "fifteen feature distances", "d2 = dot(c_Q - c_V, c_Q - c_V)",
                   "PT(u_j; v_0, v_1, v_2): c_Q = u_j, c_V = x", "PT(v_j; u_0, u_1, u_2): c_Q = x, c_V = v_j", "(0,0), (1,0), (0,1)",
                   "features 6 + 3 i + j (i, j = 0, 1, 2, i outer): SS(u_i, u_(i+1)%3; v_j, v_(j+1)%3): c_Q = x, c_V = y",
                   "(tv, 0) for j = 0, (1 - tv, tv) for j = 1 and (0, 1 - tv) for j = 2", "m = +inf", "takes over when its d2 < m",
                   "dist2 = 0 when the pair overlaps by rt_triangle_overlap_device's definition (its steps 1 to 4, unchanged)",
                   "(double)rmax_i * (double)rmax_i (exact) when rmax_i > 0", "a NaN, zero or negative radius is an empty search",
                   "lexicographic (dist2, triangle index) minimum over the candidates with dist2 < bound2_i", "a NaN dist2 never wins",
                   "distance = sqrtf((float)dist2)", "(float)((double)Q_0[a] + c[a])", "37 * 2^-53 * M"):
        assert phrase in doc, phrase


def _scene_of(T):
    V = np.ascontiguousarray(np.asarray(T, F32).reshape(-1, 3))
    return V, np.arange(len(V), dtype=np.uint32).reshape(-1, 3)


def _pairs(A, B):
    """Pair i is (A[i], B[i]): the restatement's (dist2, cq, cv) per pair, witnesses as absolute float64 coordinates."""
    A, B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
    q0 = A[:, 0].astype(F64)
    u, v = A.astype(F64) - q0[:, None], B.astype(F64) - q0[:, None]
    m, f, pa, pb, cq, cv = DR.pair_features(u, v)
    V, tri = _scene_of(B)
    over = np.array([TR.overlap_matrix(A[i:i + 1], V, tri[i:i + 1])[0, 0] for i in range(len(A))])
    return np.where(over, 0.0, m), m, cq + q0, cv + q0


def _exact_point_triangle2(p, T) -> Fraction:
    """The exact squared distance from the float64 point p to the float32 triangle T."""
    fr = [[Fraction(float(x)) for x in q] for q in [p] + [list(t) for t in T]]
    den = max(x.denominator for q in fr for x in q)
    ints = [tuple(int(x * den) for x in q) for q in fr]
    return Fraction(DR._exact_pt(ints[0], ints[1], ints[2], ints[3])) / (den * den)


def _check_against_exact(A, B, what, witnesses=40):
    """dist2 == 0 exactly where the exact test says overlap; elsewhere |sqrt(dist2) - d| <= c 2^-53 M; on `witnesses`
    of the pairs the witnesses lie on their triangles and are sqrt(dist2) apart, within the same bound. Returns the
    worst |sqrt(dist2) - d| / (2^-53 M) and the exact verdicts."""
    A, B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
    V, tri = _scene_of(B)
    assert IR.candidates(V, tri).all() and TR.query_valid(A).all(), what
    d2, m, cq, cv = _pairs(A, B)
    worst, exact0 = 0.0, np.zeros(len(A), bool)
    for i in range(len(A)):
        e2 = DR.exact_dist2(A[i], B[i])
        exact0[i] = e2 == 0
        unit = EPS * DR.bound_m(A[i], B[i])
        if e2 == 0:
            assert d2[i] == 0.0, f"{what}: pair {i} overlaps exactly, dist2 {d2[i]!r}"
            continue
        assert d2[i] > 0.0, f"{what}: pair {i} is {math.sqrt(e2)} apart exactly, dist2 0: {A[i]}, {B[i]}"
        ratio = abs(math.sqrt(d2[i]) - math.sqrt(e2)) / unit
        worst = max(worst, ratio)
        assert ratio <= DR.C_PROOF, f"{what}: pair {i}: sqrt(dist2) {math.sqrt(d2[i])!r}, exact {math.sqrt(e2)!r}, {ratio:.1f} units"
    for i in range(0, len(A), max(1, len(A) // witnesses)):
        unit = EPS * DR.bound_m(A[i], B[i])
        on_q, on_v = math.sqrt(_exact_point_triangle2(cq[i], A[i])), math.sqrt(_exact_point_triangle2(cv[i], B[i]))
        assert on_q <= DR.C_PROOF * unit and on_v <= DR.C_PROOF * unit, f"{what}: pair {i}: witnesses {on_q / unit:.1f}, {on_v / unit:.1f} units off"
        apart = math.sqrt(sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(cq[i], cv[i])))
        assert abs(apart - math.sqrt(m[i])) <= DR.C_PROOF * unit, f"{what}: pair {i}: witnesses {apart!r} apart, sqrt(m) {math.sqrt(m[i])!r}"
    return worst, exact0


def _lattice_sets():
    """The three lattice sets of tests/test_triangle_overlap_ref.py (the same generators and seed), in units of 1/16."""
    import test_triangle_overlap_ref as TOR
    rng = np.random.default_rng(1)
    A = TOR._lattice_triangles(rng, 1200)
    B = np.clip(A[:, :1] + rng.integers(-20, 21, (1200, 3, 3)), -48, 48)
    keep = np.array([bool(np.any(np.cross(b[1] - b[0], b[2] - b[0]))) for b in B])
    sets = {"generic": (A[keep], B[keep])}
    A2, B2 = [], []
    for t in TOR._lattice_triangles(rng, 1600, spread=6):
        q = TOR._in_plane_lattice(rng, t)
        if q is not None:
            A2.append(q)
            B2.append(t)
    sets["coplanar"] = (np.array(A2), np.array(B2))
    A3, B3 = [], []
    for i, t in enumerate(TOR._lattice_triangles(rng, 1300, spread=8)):
        q = TOR._lattice_triangles(rng, 1, spread=8)[0]
        kind = i % 3
        if kind == 0:
            q[rng.integers(0, 3)] = t[rng.integers(0, 3)]
        elif kind == 1:
            q[0], q[1] = t[1], t[2]
        else:
            q[0] = t[0] + rng.integers(-1, 3) * (t[1] - t[0])
        if np.abs(q).max() <= 48 and np.any(np.cross(q[1] - q[0], q[2] - q[0])):
            A3.append(q)
            B3.append(t)
    sets["touching"] = (np.array(A3), np.array(B3))
    return sets


def test_lattice_pairs_against_the_exact_distance():
    total = 0
    for what, (A, B) in _lattice_sets().items():
        worst, exact0 = _check_against_exact(A / 16.0, B / 16.0, f"{what} lattice pairs")
        print(f"{what} lattice pairs: {len(A)}, {int(exact0.sum())} overlap, worst |sqrt(dist2) - d| = {worst:.2f} * 2^-53 M")
        assert len(A) >= 1000
        total += len(A)
    assert total >= 3000


def test_generic_binary32_pairs_against_the_exact_distance():
    """Around the origin and far from it: 1,000 pairs each, every pair."""
    total = apart = 0
    for seed, shift in ((3, np.zeros(3)), (4, np.array([37.0, -92.0, 13.0])), (5, np.array([-1000.0, 3.0, 513.0]))):
        rng = np.random.default_rng(seed)
        ctr = rng.uniform(-1, 1, (1000, 1, 3))
        A = (ctr + rng.uniform(-0.6, 0.6, (1000, 3, 3)) * rng.choice([1.0, 0.3], (1000, 1, 1)) + shift).astype(F32)
        B = (ctr + rng.uniform(-1.2, 1.2, (1000, 1, 3)) + rng.uniform(-0.6, 0.6, (1000, 3, 3)) + shift).astype(F32)
        worst, exact0 = _check_against_exact(A, B, f"generic pairs around {shift.tolist()}")
        print(f"generic pairs around {shift.tolist()}: {int(exact0.sum())} overlap, worst {worst:.2f} * 2^-53 M")
        total += len(A)
        apart += int((~exact0).sum())
    assert total == 3000 and apart >= 1000


def _parallel_pairs():
    """Pairs with a translated copy, an edge parallel to an edge, or an edge on the other's edge line (multiples of 1/8)."""
    rng = np.random.default_rng(6)
    A, B = [], []
    for i in range(600):
        t = rng.integers(-24, 25, (3, 3)).astype(F64) / 8.0
        if not np.any(np.cross(t[1] - t[0], t[2] - t[0])):
            continue
        kind = i % 3
        if kind == 0:                                            # a translated copy: all nine edge pairs parallel
            q = t + rng.integers(-16, 17, 3) / 8.0
        elif kind == 1:                                          # one edge parallel to t's first, the third vertex anywhere
            o = rng.integers(-24, 25, 3) / 8.0
            q = np.array([o, o + rng.integers(1, 4) * (t[1] - t[0]) / 2.0, rng.integers(-24, 25, 3) / 8.0])
        else:                                                    # one edge on the line of t's first edge, past its end
            k = rng.integers(2, 5)
            q = np.array([t[0] + k * (t[1] - t[0]), t[0] + (k + 1) * (t[1] - t[0]), rng.integers(-24, 25, 3) / 8.0])
        if np.any(np.cross(q[1] - q[0], q[2] - q[0])):
            A.append(q)
            B.append(t)
    return np.array(A), np.array(B)


def test_parallel_and_collinear_edges():
    """Pairs whose nearest features are parallel edges (a zero denominator), collinear edges, and translated copies
    (every edge pair parallel), on exactly representable coordinates and on generic ones."""
    A, B = _parallel_pairs()
    assert len(A) >= 500
    worst, exact0 = _check_against_exact(A, B, "parallel and collinear edges")
    scale = F64(1.0) / 3.0                                       # the same shapes on coordinates that round
    worst2, _ = _check_against_exact((A * scale + 0.1).astype(F32), (B * scale + 0.1).astype(F32), "parallel edges, rounded")
    print(f"parallel and collinear edges: {len(A)} pairs, {int(exact0.sum())} overlap, worst {worst:.2f} and {worst2:.2f} * 2^-53 M")
    assert (~exact0).sum() >= 100


# ---- the exact checker against another formulation -----------------------------------------------------------------
def _alt_point_segment(p, a, b) -> Fraction:
    d, w = DR._isub(b, a), DR._isub(p, a)
    t = min(max(Fraction(DR._idot(w, d), DR._idot(d, d)), Fraction(0)), Fraction(1))
    r = tuple(w[k] - t * d[k] for k in range(3))
    return DR._idot(r, r)


def _alt_point_triangle(p, a, b, c) -> Fraction:
    """The distance to the plane where the foot of the perpendicular is inside the triangle (three edge functions of
    one sign), else the nearest of the three edges as segments."""
    n = TR._crs(DR._isub(b, a), DR._isub(c, a))
    side = [DR._idot(n, TR._crs(DR._isub(y, x), DR._isub(p, x))) for x, y in ((a, b), (b, c), (c, a))]
    if min(side) >= 0:
        return Fraction(DR._idot(n, DR._isub(p, a)) ** 2, DR._idot(n, n))
    return min(_alt_point_segment(p, x, y) for x, y in ((a, b), (b, c), (c, a)))


def _alt_segment_segment(p0, p1, r0, r1) -> Fraction:
    """The four endpoint-to-segment distances, and the common perpendicular where the two lines' nearest points
    (the unclamped 2 x 2 solution) lie inside both segments."""
    best = min(_alt_point_segment(p0, r0, r1), _alt_point_segment(p1, r0, r1), _alt_point_segment(r0, p0, p1), _alt_point_segment(r1, p0, p1))
    g, h, r = DR._isub(p1, p0), DR._isub(r1, r0), DR._isub(p0, r0)
    n = TR._crs(g, h)
    nn = DR._idot(n, n)
    if nn != 0:                                                  # s, t from Cramer's rule on r + s g - t h perpendicular to g and h
        s = Fraction(-DR._idot(TR._crs(h, n), r), nn)            # (r + s g - t h = lambda n, dotted with h x n and with g x n)
        t = Fraction(-DR._idot(TR._crs(g, n), r), nn)
        if 0 <= s <= 1 and 0 <= t <= 1:
            best = min(best, Fraction(DR._idot(n, r) ** 2, nn))
    return best


def _alt_exact_dist2(A, B) -> Fraction:
    if TR.exact_overlap(A, B):
        return Fraction(0)
    a, b = TR._ints(A, B)
    scale = max(Fraction(float(x)).denominator for t in (A, B) for p in t for x in p)
    best = min([_alt_point_triangle(a[j], *b) for j in range(3)] + [_alt_point_triangle(b[j], *a) for j in range(3)] +
               [_alt_segment_segment(a[i], a[(i + 1) % 3], b[j], b[(j + 1) % 3]) for i in range(3) for j in range(3)])
    return best / (scale * scale)


def test_the_exact_checker_against_another_formulation():
    """exact_dist2 follows the case lists of the code under test in rationals (the triangle's seven regions, the
    clamped segment pair with sq = 0 for parallel ones), so an error of method would be shared. Here the same distance
    by other means: the plane distance or the nearest edge for a point, the four endpoint distances and the common
    perpendicular for two segments. Equal as rationals on every pair."""
    sets = _lattice_sets()
    pairs = [(a / 16.0, b / 16.0) for A, B in sets.values() for a, b in zip(A[::8], B[::8])]
    A, B = _parallel_pairs()
    pairs += list(zip(A[::2], B[::2]))
    rng = np.random.default_rng(8)
    ctr = rng.uniform(-1, 1, (300, 1, 3)) + np.array([37.0, -92.0, 13.0])
    pairs += list(zip((ctr + rng.uniform(-0.6, 0.6, (300, 3, 3))).astype(F32),
                      (ctr + rng.uniform(-1.2, 1.2, (300, 1, 3)) + rng.uniform(-0.6, 0.6, (300, 3, 3))).astype(F32)))
    apart = 0
    for i, (a, b) in enumerate(pairs):
        a, b = np.asarray(a, F32), np.asarray(b, F32)
        want = _alt_exact_dist2(a, b)
        assert DR.exact_dist2(a, b) == want, f"pair {i}: {a}, {b}"
        apart += want > 0
    print(f"exact checker: {len(pairs)} pairs equal to the other formulation, {apart} apart")
    assert len(pairs) >= 1000 and apart >= 500


def test_named_constructions():
    T = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    cases = {
        "vertex above the face": ([[1, 1, 0.5], [1, 1, 2], [2, 1, 3]], 0.25, (1, 1, 0.5), (1, 1, 0)),
        "scene vertex nearest to the query's face": ([[-1, -1, -2], [9, -1, -2], [-1, 9, -2]], 4.0, None, None),
        "crossed edges": ([[2, -3, 1], [2, 1, 5], [2, -3, 9]], 8.0, (2, -2, 2), (2, 0, 0)),
        "parallel planes": ([[0, 0, 0.5], [4, 0, 0.5], [0, 4, 0.5]], 0.25, (0, 0, 0.5), (0, 0, 0)),
        "piercing the face": ([[1, 1, -1], [1, 1, 1], [5, 5, 1]], 0.0, None, None),
        "shared vertex": ([[0, 0, 0], [-1, -1, 3], [-2, 1, 2]], 0.0, (0, 0, 0), (0, 0, 0)),
        "coplanar disjoint": ([[3, 3, 0], [5, 3, 0], [3, 5, 0]], 2.0, (3, 3, 0), (2, 2, 0)),
    }
    for what, (Q, want, wq, wv) in cases.items():
        d2, m, cq, cv = _pairs(np.array([Q], F32), np.array([T], F32))
        assert d2[0] == want, (what, d2[0])
        assert DR.exact_dist2(np.array(Q, F32), np.array(T, F32)) == Fraction(want), what + " (exact)"
        if wq is not None:
            assert cq[0].tolist() == list(wq) and cv[0].tolist() == list(wv), (what, cq[0], cv[0])
    # the closest point of the query's vertices alone misses the edge-edge case: the nearest vertex is farther
    assert min(DR._exact_pt(tuple(p), (0, 0, 0), (4, 0, 0), (0, 4, 0)) for p in cases["crossed edges"][0]) == 10


def test_symmetry_of_the_restatement():
    """Swapping query and candidate gives the same dist2 within the bound. Not the same bits: the coordinates are taken
    relative to the query's first vertex, so the swapped pair rounds other differences, and the features come in
    another order with other roles (SS clamps its first segment's parameter first)."""
    rng = np.random.default_rng(7)
    ctr = rng.uniform(-1, 1, (1500, 1, 3)) + np.array([20.0, -7.0, 3.0])
    A = (ctr + rng.uniform(-0.5, 0.5, (1500, 3, 3))).astype(F32)
    B = (ctr + rng.uniform(-1.0, 1.0, (1500, 1, 3)) + rng.uniform(-0.5, 0.5, (1500, 3, 3))).astype(F32)
    ab, _, cq, cv = _pairs(A, B)
    ba, _, cq2, cv2 = _pairs(B, A)
    unit = EPS * np.array([max(DR.bound_m(a, b), DR.bound_m(b, a)) for a, b in zip(A, B)])
    assert ((ab == 0) == (ba == 0)).all()
    ratio = np.abs(np.sqrt(ab) - np.sqrt(ba)) / unit
    print(f"symmetry: worst |sqrt(dist2(Q, V)) - sqrt(dist2(V, Q))| = {ratio.max():.2f} * 2^-53 M, {int((ab != ba).sum())} of 1500 differ in bits")
    assert ratio.max() <= 2 * DR.C_PROOF                          # each side is within c of the true distance
    assert (ab > 0).sum() >= 500


def test_answers_bounds_ties_and_self():
    V, tri = IR.blob()
    Q = DR.distance_queries(V, tri)[::7]
    matrix = DR.dist2_matrix(Q, V, tri)
    rec, qp, pp, within, eligible, D2 = DR.answers(Q, V, tri, matrix=matrix)
    dist = rec[:, 1].view(F32)
    hit = rec[:, 0] >= 0
    assert np.array_equal(hit, TR.query_valid(Q)) and np.array_equal(within, hit.astype(np.uint8))
    assert (rec[~hit] == DR.MISS).all() and not qp[~hit].any() and not pp[~hit].any()
    over = TR.overlap_matrix(Q, V, tri)
    assert np.array_equal(dist[hit] == 0, over[hit].any(axis=1))  # distance 0 exactly where the overlap entry lists something
    first = np.array([np.flatnonzero(o)[0] if o.any() else -1 for o in over])
    assert np.array_equal(rec[over.any(axis=1), 0], first[over.any(axis=1)])   # ... and its lowest index wins
    # a radius just above and just below the distance
    r_in = np.nextafter(dist, F32(np.inf)).astype(F32)
    r_out = dist.copy()
    rec_in, *_ = DR.answers(Q, V, tri, rmax=r_in, matrix=matrix)
    rec_out, _, _, w_out, _, _ = DR.answers(Q, V, tri, rmax=r_out, matrix=matrix)
    assert np.array_equal(rec_in[hit & (dist > 0)], rec[hit & (dist > 0)])
    assert (rec_out[dist == 0] == DR.MISS).all()                 # radius 0: an empty search
    strict = hit & (dist > 0) & (D2[np.arange(len(Q)), np.maximum(rec[:, 0], 0)] >= dist.astype(F64) ** 2)
    assert strict.sum() > 20 and (rec_out[strict, 0] != rec[strict, 0]).all()
    for bad in (np.nan, 0.0, -1.0):
        assert (DR.answers(Q, V, tri, rmax=np.full(len(Q), bad, F32), matrix=matrix)[0] == DR.MISS).all()
    # the mesh against itself with self = arange: the neighbours are passed over
    own = V[tri.astype(np.int64)][:64]
    rec_s, *_ = DR.answers(own, V, tri, self_index=np.arange(64))
    rec_n, *_ = DR.answers(own, V, tri)
    assert (rec_n[:, 1].view(F32) == 0).all() and (rec_s[:, 1].view(F32) > 0).all()
    skip = TR.self_matrix(tri, np.arange(64), 64)
    assert not skip[np.arange(64), rec_s[:, 0]].any()
