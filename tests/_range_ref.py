"""The expectation of the ranged device queries (rt_closest_hit_range_device, rt_occluded_range_device), shared
by tests/test_range_ref.py (which pins it to the oracle, on the CPU) and tests/test_gpu_range_queries.py.

`pairs` restates the oracle's ray_intersect_triangle (oracle/rt_oracle.c, raytracing.cpp:106-149) and the
distance intersectMesh compares (:182) in numpy for every ray x triangle pair: float32 arrays throughout, one
rounding per operation (numpy does not contract), the dot product as (x x' + y y') + z z'. From those the
range answers follow by the rules of include/raytracert.h: in range iff tmin <= dist < tmax, both bounds
clamped above to FLT_MAX, an empty range (a NaN bound, tmax <= 0, tmin >= tmax) a miss; the closest hit the
lexicographic (dist, index) minimum.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
SMALL_NUM = F32(0.00001)
HAS_TR = 0x20
INF_BITS = 0x7F800000


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def scene_triangles(orc) -> tuple[np.ndarray, np.ndarray]:
    """(T [nt, 3, 3] float32 vertex positions, transparent [nt] bool) of an OracleScene."""
    e = orc.export()
    T = np.ascontiguousarray(e["vertices"][e["triangles"].astype(np.int64)], F32)
    tr_mat = np.array([bool(m["flags"] & HAS_TR) and m["Tr"] < 1 for m in e["materials"]])
    return T, tr_mat[e["tri_mat"]]


def pairs(o: np.ndarray, d: np.ndarray, T: np.ndarray) -> dict:
    """Every ray against every triangle: accept [n, nt] bool; dist, s, t [n, nt] and I [n, nt, 3] float32
    (meaningful where accept)."""
    o, d, T = (np.ascontiguousarray(a, F32) for a in (o, d, T))
    assert o.dtype == d.dtype == T.dtype == F32
    with np.errstate(all="ignore"):
        ux, uy, uz = (T[None, :, 1, k] - T[None, :, 0, k] for k in range(3))
        vx, vy, vz = (T[None, :, 2, k] - T[None, :, 0, k] for k in range(3))
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        degenerate = (nx == 0) & (ny == 0) & (nz == 0)
        ox, oy, oz = (o[:, None, k] for k in range(3))
        dx, dy, dz = (d[:, None, k] - o[:, None, k] for k in range(3))
        t0x, t0y, t0z = (T[None, :, 0, k] for k in range(3))
        w0x, w0y, w0z = ox - t0x, oy - t0y, oz - t0z
        b = _dot(nx, ny, nz, dx, dy, dz)
        a = -_dot(nx, ny, nz, w0x, w0y, w0z)
        ok = ~degenerate & ~(np.abs(b) < SMALL_NUM)
        r = a / b
        ok &= ~(r < 0)
        Ix, Iy, Iz = ox + dx * r, oy + dy * r, oz + dz * r
        uu, uv, vv = _dot(ux, uy, uz, ux, uy, uz), _dot(ux, uy, uz, vx, vy, vz), _dot(vx, vy, vz, vx, vy, vz)
        wx, wy, wz = Ix - t0x, Iy - t0y, Iz - t0z
        wu, wv = _dot(wx, wy, wz, ux, uy, uz), _dot(wx, wy, wz, vx, vy, vz)
        D = uv * uv - uu * vv
        s = (uv * wv - vv * wu) / D
        ok &= ~((s < 0) | (s > 1))
        t = (uv * wu - uu * wv) / D
        ok &= ~((t < 0) | ((s + t) > 1))
        ex, ey, ez = ox - Ix, oy - Iy, oz - Iz
        dist = np.sqrt(_dot(ex, ey, ez, ex, ey, ez))
    for x in (r, s, t, dist, Ix):
        assert x.dtype == F32
    return dict(accept=ok, dist=dist, s=s, t=t, I=np.stack([Ix, Iy, Iz], axis=2))


def ray_length(o, d) -> np.ndarray:
    """|dest - origin| as RT_RANGE_TO_DEST takes it: sqrtf((dx dx + dy dy) + dz dz) in float32."""
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    with np.errstate(all="ignore"):
        e = d - o
        return np.sqrt(_dot(e[:, 0], e[:, 1], e[:, 2], e[:, 0], e[:, 1], e[:, 2]))


def bounds(o, d, tmin=None, tmax=None, to_dest=False):
    """(lo, hi, nonempty) per ray: the clamped bounds and whether the range holds anything."""
    n = len(o)
    lo = np.zeros(n, F32) if tmin is None else np.ascontiguousarray(tmin, F32).copy()
    if tmax is not None:
        hi = np.ascontiguousarray(tmax, F32).copy()
    else:
        hi = ray_length(o, d) if to_dest else np.full(n, np.inf, F32)
    with np.errstate(invalid="ignore"):
        lo = np.where(lo > FLT_MAX, FLT_MAX, lo).astype(F32)      # (a NaN stays a NaN)
        hi = np.where(hi > FLT_MAX, FLT_MAX, hi).astype(F32)
        nonempty = (lo < hi) & (hi > 0)
    return lo, hi, nonempty


def in_range(P: dict, lo, hi, nonempty) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return P["accept"] & (P["dist"] >= lo[:, None]) & (P["dist"] < hi[:, None]) & nonempty[:, None]


def closest(P: dict, lo, hi, nonempty) -> dict:
    """The hit records and points: triangle [n] int32 (-1: miss), record [n, 4] uint32 (rt_hit's bits: a miss is
    -1, +inf, 0, 0), point [n, 3] float32."""
    m = in_range(P, lo, hi, nonempty)
    key = np.where(m, P["dist"], np.inf).astype(F32)
    k = key.argmin(axis=1)                       # the first of equal distances: the lowest index
    hit = m.any(axis=1)
    rows = np.arange(len(k))
    tri = np.where(hit, k, -1).astype(np.int32)
    rec = np.zeros((len(k), 4), np.uint32)
    rec[:, 0] = tri.view(np.uint32)
    rec[:, 1] = np.where(hit, P["dist"][rows, k].view(np.uint32), INF_BITS)
    rec[:, 2] = np.where(hit, P["s"][rows, k].view(np.uint32), 0)
    rec[:, 3] = np.where(hit, P["t"][rows, k].view(np.uint32), 0)
    point = np.where(hit[:, None], P["I"][rows, k], F32(0)).astype(F32)
    return dict(triangle=tri, record=rec, point=point, distance=rec[:, 1].copy().view(F32))


def occluded(P: dict, lo, hi, nonempty, transparent: np.ndarray, any_opaque: bool) -> np.ndarray:
    """blocked [n] uint8: isShadow's rule inside the range (the closest in-range triangle is not transparent),
    or, any_opaque, some in-range accepted triangle is not transparent."""
    if any_opaque:
        return (in_range(P, lo, hi, nonempty) & ~transparent[None, :]).any(axis=1).astype(np.uint8)
    tri = closest(P, lo, hi, nonempty)["triangle"]
    return ((tri >= 0) & ~transparent[np.maximum(tri, 0)]).astype(np.uint8)


def sorted_hits(P: dict, i: int) -> list:
    """Ray i's accepted triangles at a distance below FLT_MAX as (dist, index), in lexicographic order."""
    k = np.flatnonzero(P["accept"][i] & (P["dist"][i] < FLT_MAX))
    return sorted((float(P["dist"][i, j]), int(j)) for j in k)


def nth_distance(P: dict, nth: int) -> np.ndarray:
    """Per ray the nth smallest (0-based) distance among its accepted triangles (+inf when it has fewer)."""
    key = np.where(P["accept"] & (P["dist"] < FLT_MAX), P["dist"], np.inf).astype(F32)
    return np.sort(key, axis=1)[:, nth].astype(F32)
