"""Scenes for the size-boundary tests of the Morton-order builder and the refit (tests/test_lbvh_order.py,
tests/test_gpu_lbvh_sizes.py). Plain deterministic helpers; each returns float32 vertices (nv, 3) and
uint32 triangles (nt, 3).

The three classes (bvh.cpp tri_class): tree (a padded box, a leaf slot), always (ill-conditioned, tested by
every query), never (zero area, never accepted).
"""
from __future__ import annotations

import functools

import numpy as np

import raytracert_amd as R
from raytracert_amd import scenes

import _refit_scenes as S

MATERIALS = S.TINY_MATERIALS

# a well-conditioned triangle with edges of about 0.02 (coordinates are multiples of 2^-10: lattice() needs
# every copy's edges, and so its padding, to be the same floats)
_TEMPLATE = np.array([[-8, -6, -2], [8, -5, 2], [0, 11, 1]], np.float64) / 1024.0
_PERP_AXIS = np.array([0.3, 0.5, 0.7], np.float32)   # _refit_scenes.squeeze's
_SHIFT = np.array([0.05, -0.1, 0.3], np.float32)


def _unshared(v: np.ndarray):
    n = len(v)
    return np.ascontiguousarray(v.reshape(3 * n, 3), np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def soup(n: int, seed: int, always: float = 0.0, never: float = 0.0):
    """n unshared triangles, centroids uniform in [-1, 1]^3, edges of about 0.02. A fraction `never` has the
    third vertex on the first (zero area), a fraction `always` is squeezed to a sliver as
    _refit_scenes.squeeze does; the class of each triangle is drawn from one stream, so the three classes
    interleave through triangle order."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, (n, 1, 3))
    scale = rng.uniform(0.6, 1.0, (n, 1, 1))
    jitter = rng.uniform(-0.002, 0.002, (n, 3, 3))
    draw = rng.random(n)
    v = (centre + scale * _TEMPLATE[None] + jitter).astype(np.float32)
    is_never = draw < never
    is_always = ~is_never & (draw < never + always)
    e = v[:, 1] - v[:, 0]
    perp = np.cross(e, _PERP_AXIS).astype(np.float32)
    sliver = (v[:, 0] + np.float32(0.5) * e + np.float32(1e-4) * perp).astype(np.float32)
    v[is_always, 2] = sliver[is_always]
    v[is_never, 2] = v[is_never, 0]
    assert v.dtype == np.float32
    return _unshared(v)


def soup_exact(np_: int):
    """np_ tree-class triangles and nothing else."""
    return soup(np_, 1000 + np_)


def copies(n: int):
    """n copies of one triangle: every Morton code equal, the whole order is the tie-break's."""
    v = np.tile(np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.1, 0.7, -0.2]], np.float32), (n, 1))
    return v, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def lattice(n: int):
    """n copies of the template on an 8x8 lattice in the plane z = 0.25, symmetric about the origin: the z
    axis has zero centroid extent, there are 64 distinct codes with heavy ties, and centroids on both
    sides of zero. Triangle i sits on point 29 i mod 64, so equal codes are spread through triangle order.
    Every coordinate is a multiple of 2^-10, so all copies have the same edges and the same padding."""
    p = (29 * np.arange(n)) % 64
    at = np.stack([(p % 8 - 3.5) * 0.25, (p // 8 - 3.5) * 0.25, np.full(n, 0.25)], axis=1)
    v = at[:, None, :] + _TEMPLATE[None]
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)   # exact
    return _unshared(v.astype(np.float32))


GRID = scenes.GridSpec(grid=4, slices=13, stacks=8, spacing=0.3, radius=0.1)


@functools.lru_cache(maxsize=None)
def indexed_grid(workdir: str):
    """A 4x4 grid of 13x8 spheres plus the back plane: shared vertices, more triangles than vertices (the
    soups have nv = 3 nt), more than one sort block."""
    path = scenes.write_sphere_grid(GRID, workdir, "lbvh_sizes_grid")
    with R.Scene.load(path, device=R.RT_HOST_ONLY) as sc:
        e = sc.export()
    v, t = np.ascontiguousarray(e["vertices"], np.float32), np.ascontiguousarray(e["triangles"], np.uint32)
    assert len(t) > len(v) and len(t) > 2048
    return v, t


def move(v: np.ndarray) -> np.ndarray:
    """A float32 deformation that keeps every triangle's class (the tiny-scene tests' scale and shift); the
    callers assert that the update was a refit."""
    return (np.asarray(v, np.float32) * np.float32(1.25) + _SHIFT).astype(np.float32)


def create(v, t, device: int = R.RT_HOST_ONLY, builder: str = "lbvh") -> "R.Scene":
    return R.Scene.create(v, t, np.zeros(len(t), np.uint32), MATERIALS, device=device, builder=builder)
