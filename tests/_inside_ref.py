"""The expectation of the inside queries (rt_point_inside_device, rt_signed_distance_device), shared by
tests/test_inside_ref.py (which checks it against an independent float64 winding number, on the CPU) and
tests/test_gpu_inside.py.

`crossings` restates the definition in include/raytracert.h in numpy for every point x triangle pair: the vertex
differences d_j = V_j - p in float32 (one subtraction per component), everything after in float64 (numpy does not
contract): the three edge functions E = X_i0 Y_i1 - Y_i0 X_i1, whose products are exact, the half-open crossing
rule on Y, the cover test (an odd number of crossed edges), det and num and the above test. The vertices are the
mesh's vertex array entries, so a shared vertex has the same bits in every triangle that uses it. A triangle whose
record normal u x v (float32) is (0,0,0) is no candidate, as in tests/_closest_point_ref.py.

The meshes (indexed: vertices are shared) and the point sets of both test files are made here too.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
F64 = np.float64
AXES = tuple(range(6))                   # +x, -x, +y, -y, +z, -z
AXIS_NAMES = ("+x", "-x", "+y", "-y", "+z", "-z")
EDGES = ((1, 2), (2, 0), (0, 1))         # E_j is the edge opposite vertex j
MATERIALS = [dict(Kd=(0.5, 0.5, 0.5))]


def axis_parts(axis: int):
    """(k, sg, a, b) of a direction."""
    k = axis >> 1
    return k, (-1.0 if axis & 1 else 1.0), (k + 1) % 3, (k + 2) % 3


def candidates(V: np.ndarray, tri: np.ndarray) -> np.ndarray:
    """[nt] bool: the record normal u x v, in float32 without contraction, is not (0,0,0)."""
    T = np.ascontiguousarray(np.asarray(V, F32)[np.asarray(tri, np.int64)], F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        ux, uy, uz = (T[:, 1, k] - T[:, 0, k] for k in range(3))
        vx, vy, vz = (T[:, 2, k] - T[:, 0, k] for k in range(3))
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
    assert nx.dtype == F32
    return ~((nx == 0) & (ny == 0) & (nz == 0))


def crossings(p: np.ndarray, V: np.ndarray, tri: np.ndarray, axis: int, chunk: int = 256) -> np.ndarray:
    """crossings [n] int32: per point the number of candidates that cover it and are above it along `axis`."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    V = np.ascontiguousarray(V, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    k, sg, a, b = axis_parts(axis)
    n = len(p)
    out = np.zeros(n, np.int32)
    if len(tri) == 0:
        return out
    T = V[tri]                                                   # [nt, 3, 3] float32: the shared vertices' own bits
    cand = candidates(V, tri)
    finite = np.isfinite(p).all(axis=1)
    for i in range(0, n, chunk):
        pc = p[i:i + chunk]
        with np.errstate(all="ignore"):
            d = T[None, :, :, :] - pc[:, None, None, :]          # float32, one rounding per component
            assert d.dtype == F32
            X, Y, Z = d[..., a].astype(F64), d[..., b].astype(F64), F64(sg) * d[..., k].astype(F64)
            E, crossed = [], 0
            for i0, i1 in EDGES:
                e = X[..., i0] * Y[..., i1] - Y[..., i0] * X[..., i1]
                crossed = crossed + (((Y[..., i0] <= 0) & (Y[..., i1] > 0) & (e > 0))
                                     | ((Y[..., i1] <= 0) & (Y[..., i0] > 0) & (e < 0))).astype(np.int32)
                E.append(e)
            cover = (crossed & 1) == 1
            det = (E[0] + E[1]) + E[2]
            num = (E[0] * Z[..., 0] + E[1] * Z[..., 1]) + E[2] * Z[..., 2]
            above = ((det > 0) & (num > 0)) | ((det < 0) & (num < 0))
        out[i:i + chunk] = (cover & above & cand[None, :]).sum(axis=1)
    out[~finite] = 0
    return out


def inside(cr: np.ndarray) -> np.ndarray:
    return (np.asarray(cr) & 1).astype(np.uint8)


# ---- an independent float64 winding number ---------------------------------------------------------------------
def winding_number(p: np.ndarray, V: np.ndarray, tri: np.ndarray) -> np.ndarray:
    """[n] float64: the sum of the triangles' signed solid angles (Van Oosterom and Strackee) over 4 pi."""
    p = np.asarray(p, F64).reshape(-1, 3)
    T = np.asarray(V, F64)[np.asarray(tri, np.int64)]
    A, B, Cc = (T[None, :, j, :] - p[:, None, :] for j in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, Cc))
    numer = (A * np.cross(B, Cc)).sum(-1)
    denom = la * lb * lc + (A * B).sum(-1) * lc + (A * Cc).sum(-1) * lb + (B * Cc).sum(-1) * la
    return (2.0 * np.arctan2(numer, denom)).sum(axis=1) / (4.0 * np.pi)


# ---- meshes ----------------------------------------------------------------------------------------------------
def cube():
    """(V [8, 3] float32 with coordinates 0 and 2, tri [12, 3] uint32), outward; the face z = 2 has its diagonal
    from (0,0,2) to (2,2,2), and every face's diagonal runs between its (lo, lo) and (hi, hi) corners."""
    V = np.array([[x, y, z] for x in (0, 2) for y in (0, 2) for z in (0, 2)], F32)
    ix = lambda x, y, z: (x // 2) * 4 + (y // 2) * 2 + (z // 2)
    tri = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        for c in (0, 2):
            def at(u, v):
                q = [0, 0, 0]
                q[k], q[a], q[b] = c, u, v
                return ix(*q)
            quad = [at(0, 0), at(2, 0), at(2, 2), at(0, 2)] if c == 2 else [at(0, 0), at(0, 2), at(2, 2), at(2, 0)]
            tri += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return V, np.array(tri, np.uint32)


def _octahedron(levels: int):
    V = [np.array(v, F64) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    tri = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nxt = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                q = V[i] + V[j]
                V.append(q / np.linalg.norm(q))
                mid[key] = len(V) - 1
            return mid[key]

        for i, j, k in tri:
            ij, jk, ki = m(i, j), m(j, k), m(k, i)
            nxt += [(i, ij, ki), (ij, j, jk), (ki, jk, k), (ij, jk, ki)]
        tri = nxt
    return np.array(V, F64), np.array(tri, np.uint32)


def blob():
    """An octahedron subdivided three times (512 triangles, 258 shared vertices), rotated so that no face or edge
    lines up with an axis, radially perturbed; float32. Outward, closed."""
    V, tri = _octahedron(3)
    assert V.shape == (258, 3) and tri.shape == (512, 3)
    cx, sx, cz, sz = np.cos(0.37), np.sin(0.37), np.cos(1.13), np.sin(1.13)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    V = V @ (Rz @ Rx).T
    r = 1.0 + 0.18 * np.sin(3.0 * V[:, 0] + 1.0) * np.cos(2.0 * V[:, 1]) + 0.1 * np.sin(5.0 * V[:, 2])
    return np.ascontiguousarray(V * r[:, None], F32), tri


def nested():
    """The blob and a copy scaled by 0.5 (1,024 triangles): crossings reach 4, inside is between the shells."""
    V, tri = blob()
    inner = (V * F32(0.5)).astype(F32)
    return np.concatenate([V, inner]), np.concatenate([tri, tri + np.uint32(len(V))])


def open_blob():
    """The blob with 40 triangles removed: no inside, a defined count all the same."""
    V, tri = blob()
    keep = np.ones(len(tri), bool)
    keep[np.random.default_rng(7).choice(len(tri), 40, replace=False)] = False
    return V, np.ascontiguousarray(tri[keep])


def degenerate():
    """The blob plus triangles that must never count: zero-area ones (a repeated vertex, three collinear vertices,
    a point; no candidates) and, in each coordinate plane through the blob, triangles edge-on to the two axes that
    lie in it (candidates, covered an even number of times along those)."""
    V, tri = blob()
    extra_v, extra_t = [], []

    def add(a, b, c):
        base = len(V) + len(extra_v)
        extra_v.extend([a, b, c])
        extra_t.append([base, base + 1, base + 2])

    add((0.1, 0.1, 0.1), (0.4, 0.2, 0.3), (0.4, 0.2, 0.3))
    add((-0.3, 0.0, 0.2), (0.0, 0.0, 0.2), (0.6, 0.0, 0.2))
    add((0.2, -0.2, 0.0), (0.2, -0.2, 0.0), (0.2, -0.2, 0.0))
    for k in range(3):
        for c, s in ((0.125, 0.5), (-0.25, 0.3)):
            q = [[-s, -s], [s, -0.5 * s], [0.25 * s, s]]
            pts = []
            for u, v in q:
                w = [0.0, 0.0, 0.0]
                w[k], w[(k + 1) % 3], w[(k + 2) % 3] = c, u, v
                pts.append(tuple(w))
            add(*pts)
    # a vertex of the blob reused by an edge-on triangle: shared bits with the closed surface
    base = len(V) + len(extra_v)
    extra_v.extend([(float(V[5, 0]) + 0.3, float(V[5, 1]), 0.0), (float(V[5, 0]), float(V[5, 1]), -0.4)])
    extra_t.append([5, base, base + 1])
    V2 = np.concatenate([V, np.array(extra_v, F32)]).astype(F32)
    return V2, np.concatenate([tri, np.array(extra_t, np.uint32)])


MESHES = {"cube": cube, "blob": blob, "nested": nested, "open": open_blob, "degenerate": degenerate}


# ---- points ----------------------------------------------------------------------------------------------------
def cube_grid() -> np.ndarray:
    """The 125 points of {0, 0.5, 1, 1.5, 2}^2 x {-1, 0.5, 1, 1.5, 3}."""
    xy, z = (0.0, 0.5, 1.0, 1.5, 2.0), (-1.0, 0.5, 1.0, 1.5, 3.0)
    return np.array([[x, y, w] for x in xy for y in xy for w in z], F32)


def cube_grid_classes(p: np.ndarray):
    """(strictly interior, some coordinate outside [0, 2]) of cube points."""
    return ((p > 0) & (p < 2)).all(axis=1), ((p < 0) | (p > 2)).any(axis=1)


def uniform_points(V: np.ndarray, n: int, seed: int) -> np.ndarray:
    """n float32 points uniform in 1.2 x the mesh's box."""
    v = np.asarray(V, F64)
    lo, hi = v.min(0), v.max(0)
    mid, half = (lo + hi) / 2, 1.2 * (hi - lo) / 2
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(mid - half, mid + half, (n, 3)), F32)


def under_vertex_points(V: np.ndarray, k: int, n: int, seed: int) -> np.ndarray:
    """n float32 points exactly under (or over) vertices along coordinate k: a vertex copied, coordinate k alone
    moved, so the other two differences are exactly zero."""
    rng = np.random.default_rng(seed)
    V = np.asarray(V, F32)
    p = V[rng.integers(0, len(V), n)].copy()
    lo, hi = float(V[:, k].min()), float(V[:, k].max())
    p[:, k] = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), n).astype(F32)
    return np.ascontiguousarray(p, F32)


def nonfinite_points() -> np.ndarray:
    p = np.full((6, 3), 0.1, F32)
    p[0, 0], p[1, 1], p[2, 2] = np.nan, np.inf, -np.inf
    p[3] = np.nan
    p[4, 0], p[4, 2] = np.inf, np.nan
    p[5] = np.inf
    return p


def mesh_points(name: str, V: np.ndarray) -> np.ndarray:
    """What tests/test_gpu_inside.py asks of a mesh: the cube grid (the cube), 100 points under vertices along
    each coordinate, 1,024 uniform points, and the non-finite ones."""
    parts = [cube_grid()] if name == "cube" else []
    parts += [under_vertex_points(V, k, 100, 50 + k) for k in range(3)]
    parts += [uniform_points(V, 1024, 60), nonfinite_points()]
    return np.ascontiguousarray(np.concatenate(parts), F32)
