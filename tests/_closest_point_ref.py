"""The expectation of the closest-point queries (rt_closest_point_device, rt_closest_point), shared by
tests/test_closest_point_ref.py (which checks it against an independent float64 distance, on the CPU) and
tests/test_gpu_closest_point.py.

`pairs` restates the definition in include/raytracert.h in numpy for every point x triangle pair: float32
arrays throughout, one rounding per operation (numpy does not contract), the dot product as
(x x' + y y') + z z'. Triangles come from _range_ref.scene_triangles, and a triangle whose normal u x v is
(0,0,0) is no candidate, exactly as _range_ref.pairs masks it. From the pairs follow the lexicographic
(dist2, index) minimum, the radius rule (bound = rmax * rmax in float32 when rmax > 0, else an empty search)
and the region each pair took.

The scenes and the point sets of both test files are made here too, so that the counts the CPU file asserts
(every region wins, ties occur) are counts of what the GPU file runs.
"""
from __future__ import annotations

import os

import numpy as np

import _edge_rays as E
import _query_scenes as QS
import _range_ref as RR

F32 = np.float32
INF_BITS = 0x7F800000
REGIONS = ("vertex 0", "vertex 1", "edge 0-1", "vertex 2", "edge 0-2", "edge 1-2", "interior")
V0, V1, E01, V2, E02, E12, INTERIOR = range(7)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def pairs(p: np.ndarray, T: np.ndarray) -> dict:
    """Every point against every triangle: candidate [1, nt] bool; dist2, s, t [n, nt] float32, c [n, nt, 3]
    float32, region [n, nt] int8 (an index into REGIONS)."""
    p, T = np.ascontiguousarray(p, F32), np.ascontiguousarray(T, F32)
    with np.errstate(all="ignore"):
        t0x, t0y, t0z = (T[None, :, 0, k] for k in range(3))
        ux, uy, uz = (T[None, :, 1, k] - T[None, :, 0, k] for k in range(3))
        vx, vy, vz = (T[None, :, 2, k] - T[None, :, 0, k] for k in range(3))
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        degenerate = (nx == 0) & (ny == 0) & (nz == 0)
        uu, uv, vv = _dot(ux, uy, uz, ux, uy, uz), _dot(ux, uy, uz, vx, vy, vz), _dot(vx, vy, vz, vx, vy, vz)
        px, py, pz = (p[:, None, k] for k in range(3))
        wx, wy, wz = px - t0x, py - t0y, pz - t0z
        d1, d2 = _dot(ux, uy, uz, wx, wy, wz), _dot(vx, vy, vz, wx, wy, wz)
        d3, d4 = d1 - uu, d2 - uv
        d5, d6 = d1 - uv, d2 - vv
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        q = one / ((va + vb) + vc)
        si, ti = vb * q, vc * q
        si = np.where(si < 0, zero, si)          # compares, not fmin / fmax: a NaN stays a NaN
        si = np.where(si > 1, one, si)
        m = one - si
        ti = np.where(ti < 0, zero, ti)
        ti = np.where(ti > m, m, ti)
        t12 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        conds = [
            (d1 <= 0) & (d2 <= 0),
            (d3 >= 0) & (d4 <= d3),
            (vc <= 0) & (d1 >= 0) & (d3 <= 0),
            (d6 >= 0) & (d5 <= d6),
            (vb <= 0) & (d2 >= 0) & (d6 <= 0),
            (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0),
        ]
        s = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, one - t12], si).astype(F32)
        t = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), t12], ti).astype(F32)
        region = np.select(conds, list(range(6)), INTERIOR).astype(np.int8)
        cx, cy, cz = (t0x + s * ux) + t * vx, (t0y + s * uy) + t * vy, (t0z + s * uz) + t * vz
        rx, ry, rz = px - cx, py - cy, pz - cz
        dist2 = _dot(rx, ry, rz, rx, ry, rz)
    for x in (s, t, dist2, cx):
        assert x.dtype == F32
    return dict(candidate=~degenerate, dist2=dist2, s=s, t=t, c=np.stack([cx, cy, cz], axis=2), region=region)


def bound(n: int, rmax=None) -> np.ndarray:
    """bound [n] float32: +inf without radii, rmax * rmax where rmax > 0, else -1 (nothing is below it)."""
    if rmax is None:
        return np.full(n, np.inf, F32)
    r = np.ascontiguousarray(rmax, F32)
    with np.errstate(all="ignore"):
        return np.where(r > 0, r * r, F32(-1)).astype(F32)


def closest(P: dict, rmax=None) -> dict:
    """triangle [n] int32 (-1: miss), record [n, 4] uint32 (rt_hit's bits), point [n, 3] float32, distance [n]
    float32, region [n] int8 (-1 on a miss), ties [n] bool: another candidate has the winner's dist2."""
    n = P["dist2"].shape[0]
    b = bound(n, rmax)
    with np.errstate(invalid="ignore"):
        m = P["candidate"] & (P["dist2"] < b[:, None])
    key = np.where(m, P["dist2"], np.inf).astype(F32)
    if key.shape[1] == 0:
        key = np.full((n, 1), np.inf, F32)
        m = np.zeros((n, 1), bool)
    k = key.argmin(axis=1)                       # the first of equal dist2: the lowest index
    hit = m.any(axis=1)
    rows = np.arange(n)
    tri = np.where(hit, k, -1).astype(np.int32)
    rec = np.zeros((n, 4), np.uint32)
    rec[:, 0] = tri.view(np.uint32)
    if P["dist2"].shape[1] == 0:
        rec[:, 1] = INF_BITS
        return dict(triangle=tri, record=rec, point=np.zeros((n, 3), F32), distance=rec[:, 1].copy().view(F32),
                    region=np.full(n, -1, np.int8), ties=np.zeros(n, bool))
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(P["dist2"][rows, k]).astype(F32)
    rec[:, 1] = np.where(hit, dist.view(np.uint32), INF_BITS)
    rec[:, 2] = np.where(hit, P["s"][rows, k].view(np.uint32), 0)
    rec[:, 3] = np.where(hit, P["t"][rows, k].view(np.uint32), 0)
    point = np.where(hit[:, None], P["c"][rows, k], F32(0)).astype(F32)
    ties = hit & ((m & (key == key[rows, k][:, None])).sum(axis=1) > 1)
    return dict(triangle=tri, record=rec, point=point, distance=rec[:, 1].copy().view(F32),
                region=np.where(hit, P["region"][rows, k], -1).astype(np.int8), ties=ties)


# ---- an independent float64 distance -----------------------------------------------------------------------
def true_distance(p: np.ndarray, T: np.ndarray) -> np.ndarray:
    """[n, nt] float64: the distance from each point to each triangle, as the minimum over the plane projection
    (where it falls inside the triangle) and the three clamped edge projections."""
    p = np.asarray(p, np.float64)[:, None, :]
    A, B, Cc = (np.asarray(T[:, k], np.float64)[None, :, :] for k in range(3))

    def seg(a, b):
        e = b - a
        ee = (e * e).sum(-1)
        tt = np.clip(((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        return np.linalg.norm(p - (a + tt[..., None] * e), axis=-1)

    best = np.minimum(np.minimum(seg(A, B), seg(B, Cc)), seg(Cc, A))
    nrm = np.cross(B - A, Cc - A)
    nn = (nrm * nrm).sum(-1)
    ok = nn > 0
    nn = np.where(ok, nn, 1.0)
    w = p - A
    # barycentric coordinates of the projection: inside iff all three are >= 0
    g1 = (np.cross(w, Cc - A) * nrm).sum(-1) / nn
    g2 = (np.cross(B - A, w) * nrm).sum(-1) / nn
    inside = ok & (g1 >= 0) & (g2 >= 0) & (g1 + g2 <= 1)
    plane = np.abs((w * nrm).sum(-1)) / np.sqrt(nn)
    return np.where(inside, np.minimum(best, plane), best)


def scene_m1(T: np.ndarray) -> float:
    return float(np.abs(T.astype(np.float64)).sum(axis=-1).max()) if len(T) else 0.0


# ---- scenes ---------------------------------------------------------------------------------------------------
def write_obj(directory: str, stem: str, T: np.ndarray) -> str:
    """Unshared triangles T [nt, 3, 3] float32 as an OBJ (nine significant digits: the float32 values exactly)."""
    path = os.path.join(directory, stem + ".obj")
    with open(path, "w", newline="\n") as f:
        for q in np.asarray(T, F32).reshape(-1, 3):
            f.write("v %.9g %.9g %.9g\n" % (q[0], q[1], q[2]))
        for k in range(len(T)):
            f.write("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
    return path


FAR_BASE = 1024.0            # 2^10: one ulp is 2^-13
FAR_ULP = 2.0 ** -13
N_FAR = 300


def far_tiny_triangles() -> np.ndarray:
    """300 triangles with edges of a few ulps at coordinates near 2^10 (vertices on the float32 lattice within
    +-4 ulps of centres spread over +-64 ulps), next to 6 of unit size at the origin."""
    rng = np.random.default_rng(23)
    cen = rng.integers(-64, 65, (N_FAR, 1, 3))
    off = rng.integers(-4, 5, (N_FAR, 3, 3))
    far = (FAR_BASE + (cen + off) * FAR_ULP).astype(F32)
    near = rng.uniform(-1, 1, (6, 3, 3)).astype(F32)
    return np.concatenate([far, near]).astype(F32)


def one_triangle() -> np.ndarray:
    return np.array([[[0.25, -0.5, 0.125], [1.5, 0.25, -0.375], [-0.125, 1.0, 0.75]]], F32)


def degenerate_triangles() -> np.ndarray:
    """Every triangle's normal is (0,0,0): repeated vertices, collinear vertices on an axis, a point."""
    return np.array([
        [[0, 0, 0], [1, 0, 0], [1, 0, 0]],
        [[0, 0, 0], [0, 0, 0], [0, 1, 0]],
        [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]],
        [[0, 0, 1], [0, 0, 2], [0, 0, 4]],
        [[-1, 0, 0], [1, 0, 0], [3, 0, 0]],
    ], F32)


# ---- points ---------------------------------------------------------------------------------------------------
def _unit(a):
    n = np.linalg.norm(a, axis=-1, keepdims=True)
    return a / np.where(n > 0, n, 1.0)


def points_for(T: np.ndarray, seed: int, surface=None) -> np.ndarray:
    """About 256 float32 points for triangles T: random points in 1.5 x the scene box, points on the surface
    (`surface`, else barycentric combinations), exact vertices, edge midpoints and centroids, points displaced
    along the face normal from vertices and edge midpoints and outward from them in the triangle's plane (the
    vertex and edge regions), points at 1e6 and 1e30, points with a NaN or an infinite component."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, F32)
    if len(T) == 0:
        T = one_triangle()
    T64 = T.astype(np.float64)
    lo, hi = T64.reshape(-1, 3).min(0), T64.reshape(-1, 3).max(0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    out = [mid + rng.uniform(-1.5, 1.5, (80, 3)) * half]
    if surface is None:
        k = rng.integers(0, len(T), 32)
        b = rng.dirichlet((1, 1, 1), 32)
        surface = (b[:, :, None] * T64[k]).sum(1)
    out.append(np.asarray(surface, np.float64)[:40])
    k = rng.integers(0, len(T), 24)
    A, B, Cc = T64[k, 0], T64[k, 1], T64[k, 2]
    nrm = _unit(np.cross(B - A, Cc - A))
    size = np.linalg.norm(B - A, axis=1, keepdims=True) + np.linalg.norm(Cc - A, axis=1, keepdims=True)
    cen = (A + B + Cc) / 3
    out += [A[:8], B[8:16], Cc[16:24], ((A + B) / 2)[:8], ((B + Cc) / 2)[8:16], ((Cc + A) / 2)[16:24], cen[:12]]
    h = rng.uniform(0.05, 0.5, (24, 1)) * size
    for V in (A, B, Cc):                                       # above a vertex, and away from the centroid
        out.append((V + nrm * h)[:6])
        out.append((V + _unit(V - cen) * h + nrm * h * 0.25)[6:14])
    for P0, P1, P2 in ((A, B, Cc), (B, Cc, A), (Cc, A, B)):      # above an edge midpoint, and away from the third vertex
        m = (P0 + P1) / 2
        e = _unit(P1 - P0)
        away = m - P2
        away = _unit(away - (away * e).sum(1, keepdims=True) * e)
        out.append((m + nrm * h)[14:18])
        out.append((m + away * h + nrm * h * 0.25)[16:24])
    far = np.array([[1e6, 0, 0], [0, -1e6, 1e6], [1e30, 0, 0], [-1e30, 1e30, 1e30], [3e5, 2e5, -1e6], [0, 0, 1e30]])
    out.append(far)
    pts = np.concatenate(out).astype(F32)
    bad = np.repeat(pts[:1], 8, axis=0).copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    bad[3] = np.nan
    bad[4, 0], bad[4, 2] = np.inf, np.nan
    bad[5] = np.inf
    bad[6, 1] = np.nan
    bad[7, 0] = -np.inf
    return np.ascontiguousarray(np.concatenate([pts, bad]), F32)


def near_far_points(T: np.ndarray, n: int = 4096, seed: int = 31) -> np.ndarray:
    """n random float32 points within a few edge lengths (+-24 ulps) of the far triangles' vertices."""
    rng = np.random.default_rng(seed)
    v = T[:N_FAR].reshape(-1, 3).astype(np.float64)
    k = rng.integers(0, len(v), n)
    return np.ascontiguousarray(v[k] + rng.uniform(-24, 24, (n, 3)) * FAR_ULP, F32)


def in_box_points(T: np.ndarray, n: int = 256, seed: int = 41) -> np.ndarray:
    """n float32 points uniform in the triangles' bounding box."""
    rng = np.random.default_rng(seed)
    v = np.asarray(T, np.float64).reshape(-1, 3)
    return np.ascontiguousarray(rng.uniform(v.min(0), v.max(0), (n, 3)), F32)


def q_surface_points(T: np.ndarray) -> np.ndarray:
    """The hit points of ray set R200 on scene Q, by the ray restatement."""
    o, d = QS.r200()
    res = RR.closest(RR.pairs(o, d, T), *RR.bounds(o, d))
    return res["point"][res["triangle"] >= 0]


def shingles_triangles() -> np.ndarray:
    return E.triangles()
