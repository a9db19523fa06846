"""Scene "shingles" and the edge-ray classes shared by tests/test_edge_rays.py (what the oracle alone says
about them) and tests/test_gpu_edge_rays.py (every traversal against the oracle, bit for bit).

Scene: 701 unshared triangles (not a multiple of 64), centroids uniform in [-1, 1]^3, vertices centroid +
N(0, 0.35) in float32 (default_rng(5)): big overlapping boxes, so a ray is accepted by several triangles and
the first leaf a walk reaches often does not hold the nearest hit: a wrong distance cull shows. Two material
names alternate over the triangles; in `shingles` both are opaque, in `shingles_tr` the second is transparent
(d 0.5), so rt_occluded_device takes the closest-hit walk there. Coordinates are written with nine
significant digits, so the file holds the float32 values exactly, also scaled by a power of two (scale=...).

Ray classes, each a float32 (origins, dests) pair (the reference's ray is dest - origin):
  A generic   base rays (from the sphere of radius 3 to points of [-0.8, 0.8]^3), every fourth aimed past the scene
  B long      dest = o + (p - o) s, s = 1e20, 1e25, 1e30: dot(dir, dir) overflows
  C short     s = 1e-2, 1e-4, 1e-6 (the last below the reference's |n.dir| < 1e-5 test: no hit)
  D axis      two direction components exactly 0 (each axis, both senses, from +-3); the same from inside;
              one component exactly +0 or -0 from an 8 x 8 grid of origins
  E zero      dest == origin, inside and outside the scene
  F far       origin s for s = 1e4, 1e7, 1e12, 1e30, dest unchanged (from 1e7 the pad exceeds the scene: every
              box is wanted, the deepest stack a walk can reach; at 1e30 the distance is not below FLT_MAX)
  G planes    origin coordinates equal to vertex coordinates, rays through vertices and along edges
  H nonfinite one or several of the six components NaN, +inf or -inf
"""
from __future__ import annotations

import os

import numpy as np

N_TRI = 701
SCENE_SEED = 5
RAY_SEED = 5
N_BASE = 256
BIG = float(2 ** 21)           # the exact scale at which scene_m1 >= 1e6 (the binary tree is the default walk)
MID = float(2 ** 10)           # scene_m1 < 1e6 (the four-wide walk), and n.dir of the longest rays overflows
B_SCALES = (1e20, 1e25, 1e30)
C_SCALES = (1e-2, 1e-4, 1e-6)
F_SCALES = (1e4, 1e7, 1e12, 1e30)
PREFIXES = (1, 63, 64, 65)
F32 = np.float32


def triangles() -> np.ndarray:
    """[N_TRI, 3, 3] float32 vertex positions."""
    rng = np.random.default_rng(SCENE_SEED)
    cen = rng.uniform(-1, 1, (N_TRI, 1, 3))
    return (cen + rng.standard_normal((N_TRI, 3, 3)) * 0.35).astype(F32)


def write_scene(directory: str, stem: str, transparent: bool = False, scale: float = 1.0) -> str:
    """The OBJ/MTL pair; returns the OBJ path."""
    v = (triangles() * F32(scale)).astype(F32).reshape(-1, 3)
    with open(os.path.join(directory, stem + ".mtl"), "w", newline="\n") as f:
        for name, kd, tr in (("Slate", (0.7, 0.3, 0.2), False), ("Pane", (0.2, 0.5, 0.8), transparent)):
            f.write(f"newmtl {name}\nNs 96.078431\nKa 0.000000 0.000000 0.000000\nKd %.6f %.6f %.6f\n" % kd)
            f.write("Ks 0.500000 0.500000 0.500000\n")
            f.write("Ni 1.500000\nd 0.500000\n" if tr else "Ni 1.000000\nd 1.000000\n")
            f.write("illum 2\n\n")
    path = os.path.join(directory, stem + ".obj")
    with open(path, "w", newline="\n") as f:
        f.write(f"mtllib {stem}.mtl\n")
        for p in v:
            f.write("v %.9g %.9g %.9g\n" % (p[0], p[1], p[2]))
        for t in range(N_TRI):
            f.write("usemtl %s\nf %d %d %d\n" % ("Pane" if t % 3 == 2 else "Slate", 3 * t + 1, 3 * t + 2, 3 * t + 3))
    return path


def _sphere(rng, n: int, radius: float) -> np.ndarray:
    x = rng.standard_normal((n, 3))
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * radius).astype(F32)


def base_rays() -> tuple[np.ndarray, np.ndarray]:
    """N_BASE rays from the sphere of radius 3 to uniform points of [-0.8, 0.8]^3."""
    rng = np.random.default_rng(RAY_SEED)
    o = _sphere(rng, N_BASE, 3.0)
    p = rng.uniform(-0.8, 0.8, (N_BASE, 3)).astype(F32)
    return o, p


def generic() -> tuple[np.ndarray, np.ndarray]:
    o, p = base_rays()
    p = p.copy()
    # every fourth ray to a point of the radius-3 sphere about 40 degrees from its origin: past the scene
    rng = np.random.default_rng(RAY_SEED + 1)
    k = np.arange(3, N_BASE, 4)
    side = np.cross(o[k], _sphere(rng, len(k), 1.0))
    side = side / np.linalg.norm(side, axis=1, keepdims=True) * 3.0
    p[k] = (o[k] * np.cos(0.7) + side * np.sin(0.7)).astype(F32)
    return o, p


def stretched(s: float) -> tuple[np.ndarray, np.ndarray]:
    """The base rays with dest = o + (p - o) s, every step in float32."""
    o, p = base_rays()
    return o, (o + (p - o) * F32(s)).astype(F32)


def axis_outside(axis: int) -> tuple[np.ndarray, np.ndarray]:
    """256 rays along one axis (128 per sense) from +-3: the two other direction components are exactly 0."""
    rng = np.random.default_rng(RAY_SEED + 10 + axis)
    o = rng.uniform(-0.8, 0.8, (N_BASE, 3)).astype(F32)
    sense = np.where(np.arange(N_BASE) % 2 == 0, 1.0, -1.0).astype(F32)
    o[:, axis] = -3.0 * sense
    d = o.copy()
    d[:, axis] = o[:, axis] + sense
    return o, d


def axis_inside() -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(RAY_SEED + 20)
    o = rng.uniform(-0.9, 0.9, (N_BASE, 3)).astype(F32)
    return o, (o + np.array([1, 0, 0], F32)).astype(F32)


def axis_grid() -> tuple[np.ndarray, np.ndarray]:
    """One direction component exactly zero, from an 8 x 8 grid of origins in the plane z = 3: x zero, y zero,
    and each of them as -0.0 (origin coordinate +0.0, dest coordinate -0.0: -0.0 - 0.0 is -0.0), which puts the
    sign of a zero into the clamped reciprocal."""
    g = np.linspace(-0.7, 0.7, 8, dtype=F32)
    gx, gy = (a.ravel() for a in np.meshgrid(g, g))
    z3 = np.full(64, 3.0, F32)
    os_, ds_ = [], []
    for zero, neg in ((0, False), (1, False), (0, True), (1, True)):
        o = np.stack([gx, gy, z3], axis=1).astype(F32)
        d = np.stack([gx + F32(0.3), gy + F32(0.2), z3 - F32(3.0)], axis=1).astype(F32)
        if neg:
            o[:, zero] = 0.0
            d[:, zero] = -0.0
        else:
            d[:, zero] = o[:, zero]
        os_.append(o)
        ds_.append(d)
    return np.concatenate(os_), np.concatenate(ds_)


def zero_length() -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(RAY_SEED + 30)
    o = np.concatenate([rng.uniform(-0.9, 0.9, (N_BASE // 2, 3)).astype(F32), _sphere(rng, N_BASE // 2, 3.0)])
    return o, o.copy()


def far(s: float) -> tuple[np.ndarray, np.ndarray]:
    o, p = base_rays()
    return (o * F32(s)).astype(F32), p


def planes() -> tuple[np.ndarray, np.ndarray]:
    """Four groups of 64 over the triangles 0, 11, 22, ...: (1) down the z axis onto vertex 0 (the origin's x
    and y are the vertex's: the bounds of its boxes before padding); (2) from a generic origin through vertex 1;
    (3) along the edge 0 -> 1 from two edge lengths before it; (4) from vertex 0 itself to vertex 1."""
    T = triangles()[::11][:64]
    rng = np.random.default_rng(RAY_SEED + 40)
    v0, v1 = T[:, 0], T[:, 1]
    o1 = v0.copy()
    o1[:, 2] = 3.0
    o2 = _sphere(rng, 64, 3.0)
    o3 = (v0 - F32(2.0) * (v1 - v0)).astype(F32)
    return np.concatenate([o1, o2, o3, v0]).astype(F32), np.concatenate([v0, v1, v1, v1]).astype(F32)


def nonfinite() -> tuple[np.ndarray, np.ndarray]:
    """64 base rays: 54 with one of the six components NaN, +inf or -inf, 10 with several."""
    o, p = (a[:64].copy() for a in base_rays())
    r = np.concatenate([o, p], axis=1)
    vals = (np.nan, np.inf, -np.inf)
    for i in range(54):
        r[i, i % 6] = vals[(i // 6) % 3]
    nan, inf = np.nan, np.inf
    several = [(nan,) * 6, (inf, inf, inf, None, None, None), (None, None, None, -inf, inf, -inf),
               (inf, None, None, inf, None, None), (-inf, None, None, inf, None, None), (None, nan, None, None, inf, None),
               (inf, -inf, nan, None, None, None), (None, None, None, nan, nan, nan), (-inf,) * 6, (nan, None, inf, None, -inf, None)]
    for i, pat in enumerate(several):
        for k, v in enumerate(pat):
            if v is not None:
                r[54 + i, k] = v
    return np.ascontiguousarray(r[:, :3], F32), np.ascontiguousarray(r[:, 3:], F32)


def _tag(s: float) -> str:
    return ("%.0e" % s).replace("e+", "e").replace("e-0", "e-").replace("e0", "e")


def subclasses() -> dict:
    """name -> (origins, dests), in a fixed order; a name's first letter is its class."""
    out = {"A": generic()}
    for s in B_SCALES:
        out["B_" + _tag(s)] = stretched(s)
    for s in C_SCALES:
        out["C_" + _tag(s)] = stretched(s)
    for axis in range(3):
        out["D_" + "xyz"[axis]] = axis_outside(axis)
    out["D_inside"] = axis_inside()
    out["D_grid"] = axis_grid()
    out["E"] = zero_length()
    for s in F_SCALES:
        out["F_" + _tag(s)] = far(s)
    out["G"] = planes()
    out["H"] = nonfinite()
    for o, d in out.values():
        assert o.dtype == d.dtype == F32 and o.shape == d.shape
    return out


def class_rays(letter: str, scale: float = 1.0) -> tuple[np.ndarray, np.ndarray, dict]:
    """A class's subclasses concatenated (times `scale`, a power of two), and name -> slice of the rows."""
    os_, ds_, where, at = [], [], {}, 0
    for name, (o, d) in subclasses().items():
        if name[0] == letter:
            os_.append(o * F32(scale))
            ds_.append(d * F32(scale))
            where[name] = slice(at, at + len(o))
            at += len(o)
    return np.concatenate(os_).astype(F32), np.concatenate(ds_).astype(F32), where


def same_bits(a, b) -> bool:
    """Bytes equal, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def oracle_answers(orc, o: np.ndarray, d: np.ndarray) -> dict:
    """intersectMesh of every ray by the oracle, and the occlusion expected from it (_query_scenes.py)."""
    import _query_scenes as QS
    return QS.oracle_answers(orc, o, d)


def acceptances(tris: np.ndarray, o: np.ndarray, d: np.ndarray) -> np.ndarray:
    """How many triangles rayIntersectTriangle accepts, per ray (the oracle's own test, triangle by triangle)."""
    import oracle as O
    R = np.stack([o, d], axis=1)
    n = np.zeros(len(o), np.int64)
    for T in tris:
        n += O.ray_intersect_triangle_batch(R, T)[0]
    return n
