"""The expectation of the box-overlap queries (rt_box_overlap_device, rt_box_occupied_device), shared by
tests/test_box_overlap_ref.py (which checks it on the CPU against exact rational clipping) and
tests/test_gpu_box_overlap.py.

`overlap_matrix` restates the definition in include/raytracert.h in numpy for every box x triangle pair: step 1 the
raw compares of the vertices with the box's bounds, step 2 the centring c = (lo + hi) * 0.5f, h = (hi - lo) * 0.5f,
v_j = V_j - c in float32 (one rounding per operation), steps 3 and 4 (nine edge axes, the triangle's plane) in
float64 (numpy does not contract). np.min / np.max propagate a NaN and a compare with a NaN is false, so a NaN
separates nothing, as the header says. The vertices are the mesh's vertex array entries. A triangle whose record
normal u x v (float32) is (0,0,0) is no candidate, as in tests/_inside_ref.py.

`exact_overlap` is independent of all that: the triangle clipped by the box's six half-spaces (Sutherland-Hodgman)
in fractions.Fraction; a polygon that survives, possibly degenerate, means that the closed triangle meets the closed
box.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import _inside_ref as IR

F32 = np.float32
F64 = np.float64
MATERIALS = IR.MATERIALS


def box_valid(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """[n] bool: every component finite and lo <= hi on every axis."""
    lo, hi = np.asarray(lo, F32).reshape(-1, 3), np.asarray(hi, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)


def overlap_matrix(lo: np.ndarray, hi: np.ndarray, V: np.ndarray, tri: np.ndarray, chunk: int = 128) -> np.ndarray:
    """[n, nt] bool: triangle t is a candidate that overlaps box i."""
    lo = np.ascontiguousarray(lo, F32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, F32).reshape(-1, 3)
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n, nt = len(lo), len(tri)
    out = np.zeros((n, nt), bool)
    if nt == 0 or n == 0:
        return out
    T = V[tri]                                                   # [nt, 3, 3] float32: (triangle, vertex, axis)
    cand = IR.candidates(V, tri)
    valid = box_valid(lo, hi)
    for i in range(0, n, chunk):
        L, H = lo[i:i + chunk, None, :], hi[i:i + chunk, None, :]            # [m, 1, 3]
        with np.errstate(all="ignore"):
            # 1: raw compares
            sep = ((T.min(axis=1)[None] > H) | (T.max(axis=1)[None] < L)).any(axis=-1)      # [m, nt]
            # 2: binary32 centring, then widened
            c = (L + H) * F32(0.5)
            h32 = (H - L) * F32(0.5)
            v32 = T[None, :, :, :] - c[:, :, None, :]                                     # [m, nt, 3 (j), 3 (axis)]
            assert c.dtype == F32 and h32.dtype == F32 and v32.dtype == F32
            v, h = v32.astype(F64), h32.astype(F64)
            f = [v[:, :, 1] - v[:, :, 0], v[:, :, 2] - v[:, :, 1], v[:, :, 0] - v[:, :, 2]]
            # 3: nine edge axes
            for e in range(3):
                for a in range(3):
                    b, cc = (a + 1) % 3, (a + 2) % 3
                    p = f[e][..., b, None] * v[..., cc] - f[e][..., cc, None] * v[..., b]   # [m, nt, 3 (j)]
                    r = h[..., b] * np.abs(f[e][..., cc]) + h[..., cc] * np.abs(f[e][..., b])
                    sep |= (p.min(axis=-1) > r) | (p.max(axis=-1) < -r)
            # 4: the triangle's plane
            nn = [f[0][..., (a + 1) % 3] * f[1][..., (a + 2) % 3] - f[0][..., (a + 2) % 3] * f[1][..., (a + 1) % 3] for a in range(3)]
            d = (nn[0] * v[:, :, 0, 0] + nn[1] * v[:, :, 0, 1]) + nn[2] * v[:, :, 0, 2]
            r = (h[..., 0] * np.abs(nn[0]) + h[..., 1] * np.abs(nn[1])) + h[..., 2] * np.abs(nn[2])
            sep |= (d > r) | (d < -r)
        out[i:i + chunk] = ~sep & cand[None, :]
    out[~valid] = False
    return out


def lists(M: np.ndarray, k: int, after=None):
    """(tris [n, k] int32, nfound [n] int32, m [n] int32) of an overlap matrix: per box the k lowest overlapping
    indices greater than after_i in ascending order, then -1; min(m, k); m."""
    n, nt = M.shape
    after = np.full(n, -1, np.int64) if after is None else np.asarray(after, np.int64)
    M = M & (np.arange(nt)[None, :] > after[:, None])
    m = M.sum(axis=1).astype(np.int32)
    tris = np.full((n, k), -1, np.int32)
    for i in np.flatnonzero(m):
        idx = np.flatnonzero(M[i])[:k]
        tris[i, :len(idx)] = idx
    return tris, np.minimum(m, k).astype(np.int32), m


# ---- the exact checker -----------------------------------------------------------------------------------------
def _fr(x) -> Fraction:
    return Fraction(float(x))                                    # (a float is a dyadic rational: exact)


def exact_overlap(lo, hi, tri3, grow=Fraction(0)) -> bool:
    """Whether the closed triangle tri3 ([3][3] floats) meets the closed box [lo - grow, hi + grow] (grow < 0
    shrinks; a box shrunk past empty meets nothing): Sutherland-Hodgman in exact rationals."""
    poly = [tuple(_fr(x) for x in p) for p in tri3]
    g = Fraction(grow)
    for a in range(3):
        l, h = _fr(lo[a]) - g, _fr(hi[a]) + g
        if l > h:
            return False
        for bound, sign in ((l, 1), (h, -1)):                    # keep sign * (x[a] - bound) >= 0
            nxt = []
            for i, P in enumerate(poly):
                Q = poly[(i + 1) % len(poly)]
                dp, dq = sign * (P[a] - bound), sign * (Q[a] - bound)
                if dp >= 0:
                    nxt.append(P)
                if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                    t = dp / (dp - dq)
                    nxt.append(tuple(P[c] + t * (Q[c] - P[c]) for c in range(3)))
            poly = nxt
            if not poly:
                return False
    return True


# ---- meshes and boxes of the GPU tests ---------------------------------------------------------------------------
def sliver_blob():
    """The blob plus one sliver (angle at its first vertex about 0.29 degrees): a class 1 triangle, tested for
    every query outside the tree (the always list)."""
    V, tri = IR.blob()
    n = len(V)
    extra = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 0.005, 1.0]], F32)
    return np.concatenate([V, extra]).astype(F32), np.concatenate([tri, np.array([[n, n + 1, n + 2]], np.uint32)])


MESHES = dict(IR.MESHES, sliver=sliver_blob)


def empty_boxes():
    """(lo, hi) of every kind of empty box: a NaN or infinite component in either corner, lo > hi on one axis."""
    lo = np.full((10, 3), -0.25, F32)
    hi = np.full((10, 3), 0.25, F32)
    lo[0, 0] = np.nan
    hi[1, 1] = np.nan
    lo[2, 2] = -np.inf
    hi[3, 0] = np.inf
    lo[4], hi[4] = -np.inf, np.inf                               # "everything": infinite, so empty
    lo[5], hi[5] = np.nan, np.nan
    lo[6, 0], hi[6, 0] = 0.25, -0.25                             # inverted on x, y, z alone
    lo[7, 1], hi[7, 1] = 0.5, 0.25
    lo[8, 2], hi[8, 2] = np.nextafter(F32(0.25), F32(1)), 0.25
    lo[9], hi[9] = 0.25, -0.25
    return lo, hi


def mesh_boxes(V: np.ndarray, seed: int = 70):
    """What tests/test_gpu_box_overlap.py asks of a mesh, (lo, hi) float32 [n, 3]: 1,024 boxes uniform in the scene's
    box with edges from 0 to a quarter of its extent, 100 point boxes on vertices, 150 boxes with a face (each of
    the six in turn) on a vertex coordinate, the box that contains the whole mesh, 40 boxes outside the scene, and
    the empty ones."""
    V = np.asarray(V, F32)
    rng = np.random.default_rng(seed)
    vlo, vhi = V.min(0).astype(F64), V.max(0).astype(F64)
    ext = vhi - vlo
    ctr = rng.uniform(vlo, vhi, (1024, 3))
    half = rng.uniform(0, 0.125, (1024, 3)) * ext
    half[:16] = 0.0                                              # edges of exactly 0
    lo, hi = [(ctr - half).astype(F32)], [(ctr + half).astype(F32)]
    pv = V[rng.integers(0, len(V), 100)]
    lo.append(pv.copy())
    hi.append(pv.copy())
    fv = V[rng.integers(0, len(V), 150)].astype(F64)
    h2 = rng.uniform(0.01, 0.1, (150, 3)) * ext
    off = rng.uniform(-1, 1, (150, 3)) * h2
    flo, fhi = (fv + off - h2).astype(F32), (fv + off + h2).astype(F32)
    for i in range(150):                                          # one face exactly on the vertex's coordinate
        a, side = (i % 6) >> 1, i & 1
        if side:
            fhi[i, a] = F32(fv[i, a])
            flo[i, a] = min(flo[i, a], fhi[i, a])
        else:
            flo[i, a] = F32(fv[i, a])
            fhi[i, a] = max(fhi[i, a], flo[i, a])
    lo.append(flo)
    hi.append(fhi)
    lo.append((vlo - 0.5)[None].astype(F32))
    hi.append((vhi + 0.5)[None].astype(F32))
    oc = rng.uniform(vlo, vhi, (40, 3))
    ax = rng.integers(0, 3, 40)
    sg = rng.choice([-1.0, 1.0], 40)
    oc[np.arange(40), ax] = np.where(sg > 0, vhi[ax] + 0.3 * ext[ax], vlo[ax] - 0.3 * ext[ax])
    oh = rng.uniform(0, 0.1, (40, 3)) * ext
    lo.append((oc - oh).astype(F32))
    hi.append((oc + oh).astype(F32))
    elo, ehi = empty_boxes()
    lo.append(elo)
    hi.append(ehi)
    return np.ascontiguousarray(np.concatenate(lo), F32), np.ascontiguousarray(np.concatenate(hi), F32)
