"""The expectation of the multi-hit device query (rt_multi_hit_range_device), shared by tests/test_multi_hit_ref.py
(CPU) and tests/test_gpu_multi_hit.py.

Everything comes from tests/_range_ref.py's `pairs` and `in_range` (pinned to the oracle by tests/test_range_ref.py):
per ray the in-range accepted triangles in ascending lexicographic (distance, index) order, the first k of them
as rt_hit records, and how many there are.

Scene "doubled shingles": tests/_edge_rays.py's 701 triangles with every face listed three times (all faces, then
all again, then all again: a triangle's copies are 701 indices apart), so every accepted distance comes three
times and the index decides the order. Stepping by tmin = nextafter(previous distance) finds one of each three.
"""
from __future__ import annotations

import os

import numpy as np

import _edge_rays as E
import _range_ref as RR

F32 = np.float32
COPIES = 3
MISS = np.array([0xFFFFFFFF, RR.INF_BITS, 0, 0], np.uint32)


def _order(P: dict, lo, hi, nonempty):
    """(m [n, nt] bool in range, order [n, nt]: per ray the triangle indices by (distance, index), in-range first)."""
    m = RR.in_range(P, lo, hi, nonempty)
    key = np.where(m, P["dist"], np.inf).astype(F32)
    return m, np.argsort(key, axis=1, kind="stable")          # stable: equal distances keep the index order


def totals(P: dict, lo, hi, nonempty) -> np.ndarray:
    """m [n] int32: the number of in-range accepted triangles per ray."""
    return RR.in_range(P, lo, hi, nonempty).sum(axis=1).astype(np.int32)


def first_k(P: dict, lo, hi, nonempty, k: int) -> tuple[np.ndarray, np.ndarray]:
    """(records [n, k, 4] uint32, nhits [n] int32): rows [0, min(m, k)) of a ray are its first in-range accepted
    triangles' rt_hit bits in ascending (distance, index) order, the others the miss record; nhits = min(m, k)."""
    m, order = _order(P, lo, hi, nonempty)
    n, nt = m.shape
    rows = np.arange(n)
    rec = np.empty((n, k, 4), np.uint32)
    rec[:] = MISS
    for j in range(min(k, nt)):
        idx = order[:, j]
        ok = m[rows, idx]
        rec[ok, j, 0] = idx[ok].astype(np.uint32)
        for c, name in ((1, "dist"), (2, "s"), (3, "t")):
            rec[ok, j, c] = P[name][rows, idx].view(np.uint32)[ok]
    return rec, np.minimum(m.sum(axis=1), k).astype(np.int32)


def write_doubled(directory: str, stem: str, transparent: bool = False) -> str:
    """The doubled-shingles OBJ/MTL pair (materials as _edge_rays.write_scene: a copy has its original's); returns
    the OBJ path."""
    src = E.write_scene(directory, stem + "_src", transparent=transparent)
    os.replace(src[:-4] + ".mtl", os.path.join(directory, stem + ".mtl"))
    lines = open(src).read().splitlines()
    os.remove(src)
    head = [("mtllib %s.mtl" % stem) if ln.startswith("mtllib") else ln for ln in lines if not ln.startswith(("usemtl", "f "))]
    faces = [ln for ln in lines if ln.startswith(("usemtl", "f "))]
    assert len(faces) == 2 * E.N_TRI
    path = os.path.join(directory, stem + ".obj")
    with open(path, "w", newline="\n") as f:
        f.write("\n".join(head + faces * COPIES) + "\n")
    return path
