"""The expectation of the triangle-overlap queries (rt_triangle_overlap_device, rt_triangle_collides_device), shared
by tests/test_triangle_overlap_ref.py (which checks it on the CPU against an exact integer test) and
tests/test_gpu_triangle_overlap.py.

`overlap_matrix` restates the definition in include/raytracert.h in numpy for every query x triangle pair: step 0 the
non-finite queries, step 1 the raw compares of the candidate's vertices with the query's bounds, step 2 the widening
to float64 and the subtraction of Q_0 from both triangles, step 3 the edges and the two normals (a query whose normal
is exactly zero is empty), step 4 the seventeen axes, each as "max p < min q or min p > max q" on the three
projections of either triangle (numpy does not contract). np.min / np.max propagate a NaN and a compare with a NaN is
false, so a NaN separates nothing, as the nine compares joined by && of the header do. The vertices are the mesh's
vertex array entries. A triangle whose record normal u x v (float32) is (0,0,0) is no candidate, as in
tests/_inside_ref.py. `self_matrix` is the index filter of d_self, and `lists` is the box queries'.

`exact_overlap` is independent of all that: both triangles scaled to integers (a float is a dyadic rational), then
"some edge of one triangle meets the other closed triangle", each segment against a triangle through the sign of the
endpoints' plane distances and the crossing point's three edge functions, or, when the segment lies in the
triangle's plane, by 2-D orientation tests in the projection along the normal's largest component. Python integers
do not round.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import _box_overlap_ref as BR
import _inside_ref as IR

F32 = np.float32
F64 = np.float64
MATERIALS = BR.MATERIALS
MESHES = BR.MESHES
lists = BR.lists


def _cross(x, y):
    """x cross y on the last axis, as the header spells it: [a] = x[b] * y[c] - x[c] * y[b]."""
    return np.stack([x[..., (a + 1) % 3] * y[..., (a + 2) % 3] - x[..., (a + 2) % 3] * y[..., (a + 1) % 3] for a in range(3)], axis=-1)


def query_valid(Q: np.ndarray) -> np.ndarray:
    """[n] bool: every component finite (step 0) and n_Q not exactly (0,0,0) (step 3)."""
    Q = np.asarray(Q, F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        u = Q.astype(F64) - Q.astype(F64)[:, :1]
        nq = _cross(u[:, 1] - u[:, 0], u[:, 2] - u[:, 1])
        return np.isfinite(Q).all(axis=(1, 2)) & ~(nq == 0).all(axis=1)


def step1_survivors(Q: np.ndarray, V: np.ndarray, tri: np.ndarray) -> np.ndarray:
    """[n, nt] bool: the pairs that step 1 does not separate (any triangle, candidate or not)."""
    Q = np.asarray(Q, F32).reshape(-1, 3, 3)
    T = np.ascontiguousarray(V, F32).reshape(-1, 3)[np.asarray(tri, np.int64).reshape(-1, 3)]
    with np.errstate(all="ignore"):
        qlo, qhi = Q.min(axis=1)[:, None], Q.max(axis=1)[:, None]
        return ~((T.min(axis=1)[None] > qhi) | (T.max(axis=1)[None] < qlo)).any(axis=-1)


def overlap_matrix(Q: np.ndarray, V: np.ndarray, tri: np.ndarray, chunk: int = 64) -> np.ndarray:
    """[n, nt] bool: triangle t is a candidate that overlaps query triangle i (no `self`, no `after`)."""
    Q = np.ascontiguousarray(Q, F32).reshape(-1, 3, 3)
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n, nt = len(Q), len(tri)
    out = np.zeros((n, nt), bool)
    if nt == 0 or n == 0:
        return out
    T = V[tri]                                                   # [nt, 3, 3] float32: (triangle, vertex, axis)
    cand = IR.candidates(V, tri)
    valid = query_valid(Q)
    for i in range(0, n, chunk):
        q = Q[i:i + chunk]
        with np.errstate(all="ignore"):
            # 1: raw compares
            qlo, qhi = q.min(axis=1)[:, None], q.max(axis=1)[:, None]                     # [m, 1, 3]
            sep = ((T.min(axis=1)[None] > qhi) | (T.max(axis=1)[None] < qlo)).any(axis=-1)  # [m, nt]
            # 2: binary64, relative to Q_0
            q0 = q[:, 0].astype(F64)                                                     # [m, 3]
            u = (q.astype(F64) - q0[:, None])[:, None]                                   # [m, 1, 3 (j), 3 (axis)]
            v = T.astype(F64)[None] - q0[:, None, None]                                  # [m, nt, 3, 3]
            assert u.dtype == F64 and v.dtype == F64
            # 3: edges and normals
            e = [u[:, :, 1] - u[:, :, 0], u[:, :, 2] - u[:, :, 1], u[:, :, 0] - u[:, :, 2]]   # each [m, 1, 3]
            f = [v[:, :, 1] - v[:, :, 0], v[:, :, 2] - v[:, :, 1], v[:, :, 0] - v[:, :, 2]]   # each [m, nt, 3]
            nq, nv = _cross(e[0], e[1]), _cross(f[0], f[1])
            # 4: the seventeen axes
            axes = [nq, nv] + [_cross(e[a], f[b]) for a in range(3) for b in range(3)]
            axes += [_cross(nq, e[a]) for a in range(3)] + [_cross(nv, f[b]) for b in range(3)]
            assert len(axes) == 17
            for w in axes:
                w = w[:, :, None, :]                                                     # [m, nt or 1, 1, 3]
                p = (w[..., 0] * u[..., 0] + w[..., 1] * u[..., 1]) + w[..., 2] * u[..., 2]   # [m, nt or 1, 3 (j)]
                r = (w[..., 0] * v[..., 0] + w[..., 1] * v[..., 1]) + w[..., 2] * v[..., 2]   # [m, nt, 3]
                sep |= (p.max(axis=-1) < r.min(axis=-1)) | (p.min(axis=-1) > r.max(axis=-1))
        out[i:i + chunk] = ~sep & cand[None, :]
    out[~valid] = False
    return out


def self_matrix(tri: np.ndarray, self_index, n: int) -> np.ndarray:
    """[n, nt] bool: candidate t is passed over for query i: self_i in [0, nt) and t == self_i or t shares a vertex
    index with it. None, and any value outside [0, nt), pass nothing over."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nt = len(tri)
    skip = np.zeros((n, nt), bool)
    if self_index is None or nt == 0:
        return skip
    s = np.asarray(self_index, np.int64)[:n]
    for i in np.flatnonzero((s >= 0) & (s < nt)):
        skip[i] = np.isin(tri, tri[s[i]]).any(axis=1)
        skip[i, s[i]] = True
    return skip


# ---- the exact checker -----------------------------------------------------------------------------------------
def _ints(*tris):
    """The triangles' coordinates as Python integers on one power-of-two scale."""
    fr = [[[Fraction(float(x)) for x in p] for p in t] for t in tris]
    den = max(x.denominator for t in fr for p in t for x in p)
    return [[tuple(int(x * den) for x in p) for p in t] for t in fr]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _crs(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _sgn(x):
    return (x > 0) - (x < 0)


def _seg_seg_2d(p, q, a, b):
    """Closed segments pq and ab in the plane."""
    d1, d2, d3, d4 = _sgn(_orient(a, b, p)), _sgn(_orient(a, b, q)), _sgn(_orient(p, q, a)), _sgn(_orient(p, q, b))
    if d1 * d2 < 0 and d3 * d4 < 0:
        return True

    def on(a, b, c):                                             # c collinear with ab: within its bounds
        return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])
    return (d1 == 0 and on(a, b, p)) or (d2 == 0 and on(a, b, q)) or (d3 == 0 and on(p, q, a)) or (d4 == 0 and on(p, q, b))


def _in_tri_2d(p, t):
    s = [_sgn(_orient(t[i], t[(i + 1) % 3], p)) for i in range(3)]
    return not (min(s) < 0 and max(s) > 0)


def _seg_tri(P, Q, T):
    """The closed segment PQ meets the closed triangle T (not degenerate), in integers."""
    n = _crs(_sub(T[1], T[0]), _sub(T[2], T[0]))
    dp, dq = _dot(n, _sub(P, T[0])), _dot(n, _sub(Q, T[0]))
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return False
    if dp == 0 and dq == 0:                                      # in the triangle's plane: 2-D
        k = max(range(3), key=lambda a: abs(n[a]))
        a, b = (k + 1) % 3, (k + 2) % 3
        p2, q2, t2 = (P[a], P[b]), (Q[a], Q[b]), [(v[a], v[b]) for v in T]
        return _in_tri_2d(p2, t2) or _in_tri_2d(q2, t2) or any(_seg_seg_2d(p2, q2, t2[i], t2[(i + 1) % 3]) for i in range(3))
    D = dp - dq                                                  # X = P + (Q - P) dp / D; all of it times D
    XD = tuple(P[a] * D + (Q[a] - P[a]) * dp for a in range(3))
    s = [_sgn(_dot(n, _crs(_sub(T[(i + 1) % 3], T[i]), _sub(XD, tuple(c * D for c in T[i]))))) * _sgn(D) for i in range(3)]
    return min(s) >= 0


def exact_overlap(A, B) -> bool:
    """Whether the closed triangles A and B ([3][3] floats each, neither degenerate) have a point in common."""
    a, b = _ints(A, B)
    return any(_seg_tri(a[i], a[(i + 1) % 3], b) for i in range(3)) or any(_seg_tri(b[i], b[(i + 1) % 3], a) for i in range(3))


def exact_degenerate(A) -> bool:
    """Whether triangle A has zero area, exactly."""
    a, = _ints(A)
    return _crs(_sub(a[1], a[0]), _sub(a[2], a[0])) == (0, 0, 0)


# ---- queries of the GPU tests ------------------------------------------------------------------------------------
def nonfinite_queries() -> np.ndarray:
    q = np.tile(np.array([[-0.25, -0.25, 0.0], [0.25, -0.25, 0.1], [0.0, 0.25, -0.1]], F32), (7, 1, 1))
    q[0, 0, 0], q[1, 1, 1], q[2, 2, 2] = np.nan, np.inf, -np.inf
    q[3, 0] = np.nan
    q[4] = np.nan
    q[5, 1], q[5, 2] = -np.inf, np.inf
    q[6, 2, 0] = np.nan
    return q


def zero_area_queries(V: np.ndarray) -> np.ndarray:
    """Queries whose n_Q is exactly zero: a point in the middle of the mesh's box, a repeated vertex (each pair), and
    around the origin three collinear points with exactly representable steps."""
    c = ((np.asarray(V, F64).min(0) + np.asarray(V, F64).max(0)) * 0.5).astype(F32)
    d = np.array([0.25, 0.125, -0.5], F32)
    a, b = c, (c.astype(F64) + d).astype(F32)
    q = np.array([[a, a, a], [a, a, b], [a, b, a], [b, a, a], [a, b, b]], F32)
    o = np.zeros(3, F32)
    line = np.array([[o, d, F32(2) * d], [d, o, -d]], F32)       # collinear through the origin, exact
    return np.concatenate([q, line])


def spanning_query(V: np.ndarray, tri: np.ndarray, rng) -> np.ndarray:
    """One triangle far larger than the mesh through the middle of its box, [3, 3] float32: of 64 random planes the
    one with the most scene triangles that have vertices on both sides of it."""
    v = np.asarray(V, F64)
    mid, ext = (v.min(0) + v.max(0)) * 0.5, (v.max(0) - v.min(0)).max()
    best, best_cut = None, -1
    for _ in range(64):
        n = rng.standard_normal(3)
        n /= np.linalg.norm(n)
        side = ((v - mid) @ n > 0)[np.asarray(tri, np.int64)]
        cut = int((side.any(axis=1) & ~side.all(axis=1)).sum())
        if cut > best_cut:
            a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
            a /= np.linalg.norm(a)
            b = np.cross(n, a)
            best, best_cut = mid + 4 * ext * np.array([a, -0.5 * a + 0.9 * b, -0.5 * a - 0.9 * b]), cut
    return best.astype(F32)


def mesh_queries(V: np.ndarray, tri: np.ndarray, seed: int = 90) -> np.ndarray:
    """What tests/test_gpu_triangle_overlap.py asks of a mesh, [n, 3, 3] float32: 1,024 random triangles (centres
    uniform in the scene's box, vertices within 0.02, 0.1 and 0.3 of its extent), the triangle that cuts the whole mesh
    through its middle, 50 copies of scene triangles and 50 of them shifted along their plane, 50 triangles that share
    one vertex and 50 that share one edge with a scene triangle, the non-finite and the zero-area queries, and 40
    triangles outside the scene."""
    V = np.asarray(V, F32)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    vlo, vhi = V.min(0).astype(F64), V.max(0).astype(F64)
    ext = vhi - vlo
    ctr = rng.uniform(vlo, vhi, (1024, 1, 3))
    size = np.repeat([0.02, 0.1, 0.3, 0.1], 256)[:, None, None]
    parts = [(ctr + rng.uniform(-1, 1, (1024, 3, 3)) * size * ext).astype(F32)]
    parts.append(spanning_query(V, tri, rng)[None])
    cand = np.flatnonzero(IR.candidates(V, tri))
    T = V[tri[cand[rng.integers(0, len(cand), 200)]]]            # [200, 3, 3]
    parts.append(T[:50].copy())
    sh = T[50:100].astype(F64)
    parts.append((sh + (rng.uniform(-0.6, 0.6, (50, 1, 1)) * (sh[:, 1:2] - sh[:, 0:1]) +
                        rng.uniform(-0.6, 0.6, (50, 1, 1)) * (sh[:, 2:3] - sh[:, 0:1]))).astype(F32))
    one = T[100:150].copy()                                      # one vertex shared, the other two elsewhere
    one[:, 1:] = (one[:, :1].astype(F64) + rng.uniform(-0.15, 0.15, (50, 2, 3)) * ext).astype(F32)
    parts.append(one[:, rng.permutation(3)])
    two = T[150:200].copy()                                      # one edge shared
    two[:, 2] = (two[:, 0].astype(F64) + rng.uniform(-0.15, 0.15, (50, 3)) * ext).astype(F32)
    parts.append(two[:, [2, 0, 1]])
    parts.append(nonfinite_queries())
    parts.append(zero_area_queries(V))
    oc = rng.uniform(vlo, vhi, (40, 3))
    ax = rng.integers(0, 3, 40)
    sg = rng.choice([-1.0, 1.0], 40)
    oc[np.arange(40), ax] = np.where(sg > 0, vhi[ax] + 0.3 * ext[ax], vlo[ax] - 0.3 * ext[ax])
    parts.append((oc[:, None] + rng.uniform(-0.1, 0.1, (40, 3, 3)) * ext).astype(F32))
    return np.ascontiguousarray(np.concatenate(parts), F32)
