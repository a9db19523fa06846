"""The expectation of the triangle-distance queries (rt_triangle_distance_device, rt_triangle_within_device), shared
by tests/test_triangle_distance_ref.py (which checks it on the CPU against an exact rational distance) and
tests/test_gpu_triangle_distance.py.

`pair_features` restates the definition in include/raytracert.h in numpy float64 for arrays of pairs: PT (a point
against a triangle, rt_closest_point_device's case analysis in binary64), SS (the clamped closest points of two
segments, parallel segments starting from sq = 0) and the fifteen features in the header's order, each taking over
when its d2 is strictly below the minimum so far. numpy does not contract, np.where keeps a NaN through the clamps,
and np.select takes the first case that holds, as the header's list does. `dist2_matrix` evaluates every query x
triangle pair: u_j = Q_j - Q_0 and v_j = V_j - Q_0 in float64, the feature minimum, and 0 instead where
_triangle_overlap_ref.overlap_matrix (the overlap entry's restatement, steps 1 to 4) says the pair overlaps.
`answers` picks the lexicographic (dist2, index) minimum below the bound among the candidates that `self` does not
pass over and builds the records, the two point outputs and the verdicts from the winner's features.

`exact_dist2` is independent of the float arithmetic: both triangles scaled to integers, the same fifteen feature
pairs by exact projection in rationals (fractions.Fraction), and 0 where _triangle_overlap_ref.exact_overlap holds.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import _inside_ref as IR
import _triangle_overlap_ref as TR

F32 = np.float32
F64 = np.float64
MESHES = TR.MESHES
MATERIALS = TR.MATERIALS
mesh_queries = TR.mesh_queries
self_matrix = TR.self_matrix
overlap_matrix = TR.overlap_matrix
C_PROOF = 37.0                       # the proof's constant as the header promises it (derived: 36.5; DESIGN.md §7 "Triangle-distance
                                     # queries"); the kernel's cull uses the round 64 above it, which nothing here asserts
MISS = np.array([-1, 0x7F800000, 0, 0], np.int32)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _clamp01(x):
    x = np.where(x < 0, 0.0, x)
    return np.where(x > 1, 1.0, x)


def _pt(p, a, b, c):
    """PT(p; a, b, c) on [..., 3] float64 arrays: (s, t, x)."""
    ab, ac, w = b - a, c - a, p - a
    d1, d2 = _dot(ab, w), _dot(ac, w)
    uu, uv, vv = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
    d3, d4 = d1 - uu, d2 - uv
    d5, d6 = d1 - uv, d2 - vv
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    cases = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    t12 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    q = 1.0 / ((va + vb) + vc)
    si, ti = vb * q, vc * q
    si = np.where(si < 0, 0.0, si)
    si = np.where(si > 1, 1.0, si)
    m = 1.0 - si
    ti = np.where(ti < 0, 0.0, ti)
    ti = np.where(ti > m, m, ti)
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    s = np.select(cases, [zero, one, d1 / (d1 - d3), zero, zero, 1.0 - t12], si)
    t = np.select(cases, [zero, zero, zero, one, d2 / (d2 - d6), t12], ti)
    return s, t, (a + s[..., None] * ab) + t[..., None] * ac


def _ss(p0, p1, r0, r1):
    """SS(p0, p1; r0, r1): (sq, tv, x, y)."""
    g, h, r = p1 - p0, r1 - r0, p0 - r0
    a, e, f, c, b = _dot(g, g), _dot(h, h), _dot(h, r), _dot(g, r), _dot(g, h)
    den = a * e - b * b
    sq = np.where(den != 0, _clamp01((b * f - c * e) / den), 0.0)
    tv = (b * sq + f) / e
    lo, hi = tv < 0, tv > 1
    sq = np.where(lo, _clamp01(-c / a), np.where(hi, _clamp01((b - c) / a), sq))
    tv = np.where(lo, 0.0, np.where(hi, 1.0, tv))
    return sq, tv, p0 + sq[..., None] * g, r0 + tv[..., None] * h


def pair_features(u, v):
    """The feature minimum of pairs: u, v [..., 3 (vertex), 3 (axis)] float64, relative to Q_0 and broadcastable.
    Returns (m, f, pa, pb, cq, cv): the minimum, its feature number, its two parameters and its witnesses."""
    shape = np.broadcast_shapes(u.shape[:-2], v.shape[:-2])
    m = np.full(shape, np.inf)
    f = np.zeros(shape, np.int32)
    pa, pb = np.zeros(shape), np.zeros(shape)
    cq, cv = np.zeros(shape + (3,)), np.zeros(shape + (3,))

    def take(k, a, b, x, y):
        nonlocal m, f, pa, pb, cq, cv
        r = x - y
        d2 = _dot(r, r)
        w = d2 < m
        m, f, pa, pb = np.where(w, d2, m), np.where(w, k, f), np.where(w, a, pa), np.where(w, b, pb)
        cq, cv = np.where(w[..., None], x, cq), np.where(w[..., None], y, cv)

    with np.errstate(all="ignore"):
        for j in range(3):
            s, t, x = _pt(u[..., j, :], v[..., 0, :], v[..., 1, :], v[..., 2, :])
            take(j, s, t, np.broadcast_to(u[..., j, :], x.shape), x)
        for j in range(3):
            s, t, x = _pt(v[..., j, :], u[..., 0, :], u[..., 1, :], u[..., 2, :])
            take(3 + j, s, t, x, np.broadcast_to(v[..., j, :], x.shape))
        for i in range(3):
            for j in range(3):
                sq, tv, x, y = _ss(u[..., i, :], u[..., (i + 1) % 3, :], v[..., j, :], v[..., (j + 1) % 3, :])
                take(6 + 3 * i + j, sq, tv, x, y)
    return m, f, pa, pb, cq, cv


def record_st(f, pa, pb):
    """The candidate's barycentrics of c_V from the feature and its parameters (float64)."""
    e = (f - 6) % 3
    s = np.where(f < 3, pa, np.where(f < 6, np.where(f == 4, 1.0, 0.0), np.where(e == 0, pb, np.where(e == 1, 1.0 - pb, 0.0))))
    t = np.where(f < 3, pb, np.where(f < 6, np.where(f == 5, 1.0, 0.0), np.where(e == 0, 0.0, np.where(e == 1, pb, 1.0 - pb))))
    return s, t


def _relative(Q, T):
    """u [n, 1, 3, 3] and v [n, nt, 3, 3]: the query's and the triangles' vertices minus Q_0, float64."""
    q0 = Q[:, 0].astype(F64)
    return (Q.astype(F64) - q0[:, None])[:, None], T.astype(F64)[None] - q0[:, None, None]


def dist2_matrix(Q, V, tri, chunk: int = 64):
    """(D2 [n, nt] float64, ok [n, nt] bool): dist2 of query i and triangle t, and whether the query is not empty and
    the triangle a candidate (no `self`, no bound)."""
    Q = np.ascontiguousarray(Q, F32).reshape(-1, 3, 3)
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n, nt = len(Q), len(tri)
    D2 = np.full((n, nt), np.inf)
    ok = TR.query_valid(Q)[:, None] & IR.candidates(V, tri)[None, :]
    if n == 0 or nt == 0:
        return D2, ok
    T = V[tri]
    over = TR.overlap_matrix(Q, V, tri)
    with np.errstate(all="ignore"):
        for i in range(0, n, chunk):
            u, v = _relative(Q[i:i + chunk], T)
            D2[i:i + chunk] = pair_features(u, v)[0]
    D2[over] = 0.0
    return D2, ok


def bound2(rmax, n: int):
    """(bound2 [n] float64, searching [n] bool)."""
    if rmax is None:
        return np.full(n, np.inf), np.ones(n, bool)
    r = np.asarray(rmax, F32)[:n]
    with np.errstate(all="ignore"):
        return r.astype(F64) * r.astype(F64), r > 0


def answers(Q, V, tri, rmax=None, self_index=None, matrix=None):
    """(records [n, 4] int32, qpoints [n, 3] float32, points [n, 3] float32, within [n] uint8, eligible [n, nt] bool,
    D2): what the two entries write for these arguments. matrix: dist2_matrix(Q, V, tri), when it is at hand."""
    Q = np.ascontiguousarray(Q, F32).reshape(-1, 3, 3)
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n = len(Q)
    D2, ok = dist2_matrix(Q, V, tri) if matrix is None else matrix
    b2, searching = bound2(rmax, n)
    with np.errstate(all="ignore"):
        eligible = ok & searching[:, None] & ~self_matrix(tri, self_index, n) & (D2 < b2[:, None])
    key = np.where(eligible, D2, np.inf)
    win = key.argmin(axis=1) if key.shape[1] else np.zeros(n, np.int64)      # (the first minimum: the lowest index)
    hit = eligible.any(axis=1)
    rec = np.tile(MISS, (n, 1))
    qp, pp = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    idx = np.flatnonzero(hit)
    if idx.size:
        q = Q[idx]
        q0 = q[:, 0].astype(F64)
        u = q.astype(F64) - q0[:, None]
        v = V[tri[win[idx]]].astype(F64) - q0[:, None]
        m, f, pa, pb, cq, cv = pair_features(u, v)
        d2 = D2[idx, win[idx]]
        assert ((d2 == m) | (d2 == 0)).all()
        s, t = record_st(f, pa, pb)
        with np.errstate(all="ignore"):
            dist = np.sqrt(d2.astype(F32))
        rec[idx, 0] = win[idx]
        rec[idx, 1] = dist.astype(F32).view(np.int32)
        rec[idx, 2] = s.astype(F32).view(np.int32)
        rec[idx, 3] = t.astype(F32).view(np.int32)
        qp[idx] = (q0 + cq).astype(F32)
        pp[idx] = (q0 + cv).astype(F32)
    return rec, qp, pp, hit.astype(np.uint8), eligible, D2


# ---- the exact checker -----------------------------------------------------------------------------------------
def _isub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _idot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _point_at(a, d, s, e=None, t=0):
    return tuple(a[k] + s * d[k] + (t * e[k] if e is not None else 0) for k in range(3))


def _exact_pt(p, a, b, c):
    """The squared distance from point p to the closed triangle a b c, exactly (the Voronoi regions of the triangle)."""
    ab, ac, w = _isub(b, a), _isub(c, a), _isub(p, a)
    d1, d2 = _idot(ab, w), _idot(ac, w)
    if d1 <= 0 and d2 <= 0:
        x = a
    else:
        wb = _isub(p, b)
        d3, d4 = _idot(ab, wb), _idot(ac, wb)
        wc = _isub(p, c)
        d5, d6 = _idot(ab, wc), _idot(ac, wc)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        if d3 >= 0 and d4 <= d3:
            x = b
        elif vc <= 0 and d1 >= 0 and d3 <= 0:
            x = _point_at(a, ab, Fraction(d1, d1 - d3))
        elif d6 >= 0 and d5 <= d6:
            x = c
        elif vb <= 0 and d2 >= 0 and d6 <= 0:
            x = _point_at(a, ac, Fraction(d2, d2 - d6))
        elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
            x = _point_at(b, _isub(c, b), Fraction(d4 - d3, (d4 - d3) + (d5 - d6)))
        else:
            den = va + vb + vc
            x = _point_at(a, ab, Fraction(vb, den), ac, Fraction(vc, den))
    r = _isub(p, x)
    return _idot(r, r)


def _exact_ss(p0, p1, r0, r1):
    """The squared distance between the closed segments p0 p1 and r0 r1 (neither a point), exactly."""
    g, h, r = _isub(p1, p0), _isub(r1, r0), _isub(p0, r0)
    a, e, f, c, b = _idot(g, g), _idot(h, h), _idot(h, r), _idot(g, r), _idot(g, h)
    den = a * e - b * b
    clamp = lambda x: min(max(x, Fraction(0)), Fraction(1))
    sq = clamp(Fraction(b * f - c * e, den)) if den != 0 else Fraction(0)
    tv = (b * sq + f) / e
    if tv < 0:
        tv, sq = Fraction(0), clamp(Fraction(-c, a))
    elif tv > 1:
        tv, sq = Fraction(1), clamp(Fraction(b - c, a))
    d = _isub(_point_at(p0, g, sq), _point_at(r0, h, tv))
    return _idot(d, d)


def exact_dist2(A, B) -> Fraction:
    """The squared distance of the closed triangles A and B ([3][3] floats each, neither degenerate), exactly: 0 where
    they have a point in common, else the minimum over the fifteen feature pairs (where two disjoint triangles are
    nearest, one of them is at a vertex or both are on edges)."""
    if TR.exact_overlap(A, B):
        return Fraction(0)
    a, b = TR._ints(A, B)
    scale = max(Fraction(float(x)).denominator for t in (A, B) for p in t for x in p)
    best = min([_exact_pt(a[j], *b) for j in range(3)] + [_exact_pt(b[j], *a) for j in range(3)] +
               [_exact_ss(a[i], a[(i + 1) % 3], b[j], b[(j + 1) % 3]) for i in range(3) for j in range(3)])
    return Fraction(best) / (scale * scale)


def bound_m(A, B) -> float:
    """M of the proof for the query A and the one-triangle scene B: max_j |B_j|_1 + 2 max_j |A_j|_1."""
    return float(np.abs(np.asarray(B, F64)).sum(axis=-1).max() + 2.0 * np.abs(np.asarray(A, F64)).sum(axis=-1).max())


# ---- queries of the GPU tests ------------------------------------------------------------------------------------
def distance_queries(V, tri, seed: int = 91):
    """What tests/test_gpu_triangle_distance.py asks of a mesh, [n, 3, 3] float32: mesh_queries (random triangles of
    three sizes, the spanning one, copies of scene triangles whole, shifted, sharing a vertex and sharing an edge, the
    non-finite and zero-area queries, triangles outside the scene), then copies of 400 of the random ones shrunk to
    a tenth about their centroid and moved off by up to a fifth of the scene's extent, and 40 shrunk copies of scene
    triangles lifted off along their normal."""
    V = np.asarray(V, F32)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    base = mesh_queries(V, tri)
    rng = np.random.default_rng(seed)
    ext = (V.max(0).astype(F64) - V.min(0).astype(F64))
    src = base[rng.choice(1024, 400, replace=False)].astype(F64)
    ctr = src.mean(axis=1, keepdims=True)
    small = ctr + (src - ctr) * 0.1 + rng.uniform(-0.2, 0.2, (400, 1, 3)) * ext
    cand = np.flatnonzero(IR.candidates(V, tri))
    T = V[tri[cand[rng.integers(0, len(cand), 40)]]].astype(F64)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tc = T.mean(axis=1, keepdims=True)
    lifted = tc + (T - tc) * 0.5 + (nrm * rng.uniform(0.01, 0.1, (40, 1)) * ext.max())[:, None]
    return np.ascontiguousarray(np.concatenate([base, small.astype(F32), lifted.astype(F32)]), F32)
