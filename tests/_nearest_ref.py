"""The expectation of the nearest-triangle queries (rt_nearest_triangles_device, rt_within_radius_device), shared
by tests/test_nearest_ref.py (CPU) and tests/test_gpu_nearest.py.

The definition adds no arithmetic to the closest-point query's, so everything here is built on
_closest_point_ref.pairs (every point x triangle pair: candidate, dist2, s, t, c) and _closest_point_ref.bound
(the radius rule). Per point: the candidates with dist2 < bound, stable-sorted by dist2 (so equal dist2 stay in
ascending index order: the lexicographic (dist2, index) order), the first k of them as rt_hit rows and points,
miss rows behind them, min(m, k) and m. The scenes and point sets are that file's.
"""
from __future__ import annotations

import numpy as np

import _closest_point_ref as CP

F32 = np.float32
K_MAX = 16
KS = (1, 2, 4, 8, 16)


def admitted(P: dict, rmax=None):
    """mask [n, nt] bool: the candidates with dist2 < bound; key [n, nt] float32: their dist2, +inf elsewhere (an
    admitted dist2 is below its bound, so finite); order [n, nt]: the triangles by (key, index)."""
    n = P["dist2"].shape[0]
    b = CP.bound(n, rmax)
    with np.errstate(invalid="ignore"):
        mask = np.broadcast_to(P["candidate"], P["dist2"].shape) & (P["dist2"] < b[:, None])
    key = np.where(mask, P["dist2"], np.inf).astype(F32)
    order = np.argsort(key, axis=1, kind="stable")            # equal dist2: ascending index
    return mask, key, order


def nearest(P: dict, k: int, rmax=None) -> dict:
    """record [n, k, 4] uint32 (rt_hit's bits, miss rows 0xFFFFFFFF, +inf, 0, 0), point [n, k, 3] float32,
    triangle [n, k] int32, nfound [n] int32 = min(m, k), m [n] int32, within [n] uint8 = (m > 0), and
    cut_tie [n] bool: m > k and the dist2 at list places k and k + 1 are equal (the index alone decides which of
    the two the list holds)."""
    n, nt = P["dist2"].shape
    mask, key, order = admitted(P, rmax)
    m = mask.sum(axis=1).astype(np.int32)
    if nt < k + 1:                                            # (columns that no list place can use)
        order = np.concatenate([order, np.zeros((n, k + 1 - nt), order.dtype)], axis=1)
    sel = order[:, :k]
    rows = np.arange(n)[:, None]
    live = np.arange(k)[None, :] < np.minimum(m, k)[:, None]
    rec = np.zeros((n, k, 4), np.uint32)
    rec[..., 1] = CP.INF_BITS
    tri = np.full((n, k), -1, np.int32)
    point = np.zeros((n, k, 3), F32)
    cut_tie = np.zeros(n, bool)
    if nt:
        tri = np.where(live, sel, -1).astype(np.int32)
        safe = np.where(live, sel, 0)
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(P["dist2"][rows, safe]).astype(F32)
        rec[..., 1] = np.where(live, dist.view(np.uint32), CP.INF_BITS)
        rec[..., 2] = np.where(live, P["s"][rows, safe].view(np.uint32), 0)
        rec[..., 3] = np.where(live, P["t"][rows, safe].view(np.uint32), 0)
        point = np.where(live[..., None], P["c"][rows, safe], F32(0)).astype(F32)
        if nt > k:
            cut_tie = (m > k) & (key[rows[:, 0], order[:, k - 1]] == key[rows[:, 0], order[:, k]])
    rec[..., 0] = tri.view(np.uint32)
    return dict(record=rec, point=point, triangle=tri, nfound=np.minimum(m, k).astype(np.int32), m=m,
                within=(m > 0).astype(np.uint8), cut_tie=cut_tie)


def within(P: dict, rmax=None) -> np.ndarray:
    """[n] uint8: 1 where a candidate has dist2 < bound."""
    return (admitted(P, rmax)[0].any(axis=1)).astype(np.uint8)


def twice_closest(P: dict) -> np.ndarray:
    """rmax [n] float32: twice each point's closest distance (a miss: +inf, so twice that; a point on the mesh: 0,
    an empty search)."""
    return (F32(2) * CP.closest(P)["distance"]).astype(F32)
