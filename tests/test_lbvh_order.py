"""An independent statement of the Morton order (rt_scene_bvh_order on host-only scenes).

Every other LBVH test compares the kernels with bvh.cpp's build_lbvh, and both include lbvh_shared.h: a
wrong spread mask, clamp or float key there would pass them all. The reference here is NumPy and uses none
of that text: class and padded box per triangle from bvh_acceptance_box (the SAH builder's path), the
centroid 0.5 (lo + hi) in float32, the cell floor((c - cmin) / (cmax - cmin) * 1024) in float64 clamped to
1023 (0 on an axis without extent), the 30-bit code interleaved bit by bit with x highest, and a stable
argsort over the tree triangles in triangle order.
"""
import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi
from raytracert_amd.api import bvh_acceptance_box

import _lbvh_scenes as L
import _refit_scenes as S


def reference_order(v, t):
    """(leaf order, always list, never count, per-axis centroid extent) of the triangles t over vertices v."""
    tree, always, cen, never = [], [], [], 0
    for i, tri in enumerate(t):
        st, lo, hi = bvh_acceptance_box(v[tri])
        if st == 0:
            assert lo.dtype == np.float32 and hi.dtype == np.float32
            tree.append(i)
            cen.append(np.float32(0.5) * (lo + hi))
        elif st == 1:
            always.append(i)
        else:
            never += 1
    tree = np.array(tree, np.uint32)
    if len(tree) == 0:
        return tree, np.array(always, np.uint32), never, np.zeros(3)
    cen = np.array(cen, np.float32)
    assert cen.dtype == np.float32
    c = cen.astype(np.float64)
    cmin, cmax = c.min(axis=0), c.max(axis=0)
    code = np.zeros(len(tree), np.int64)
    cells = []
    for k in range(3):
        e = cmax[k] - cmin[k]
        if e > 0:
            q = np.minimum(np.floor((c[:, k] - cmin[k]) / e * 1024.0), 1023.0).astype(np.int64)
        else:
            q = np.zeros(len(tree), np.int64)
        assert q.min() >= 0 and q.max() <= 1023
        cells.append(q)
    for bit in range(10):
        for k in range(3):   # x highest
            code |= ((cells[k] >> bit) & 1) << (3 * bit + 2 - k)
    return tree[np.argsort(code, kind="stable")], np.array(always, np.uint32), never, cmax - cmin


def _check(v, t):
    leaf, always, never, extent = reference_order(v, t)
    with L.create(v, t) as sc:
        got_leaf, got_always = sc.bvh_order()   # (builds on demand)
        assert sc.builder == ("lbvh", "lbvh")
        info = sc.bvh_info()
        sc.bvh_validate()
    assert got_leaf.dtype == np.uint32 and got_always.dtype == np.uint32
    assert info["leaf_triangles"] == len(leaf) and info["always"] == len(always)
    assert info["never"] == never
    assert np.array_equal(got_always, always)
    assert np.array_equal(got_leaf, leaf)
    return info, extent


def test_soup_with_interleaved_classes():
    v, t = L.soup(2049, 2049, 0.03, 0.03)
    info, extent = _check(v, t)
    assert info["always"] > 20 and info["never"] > 20 and (extent > 1.5).all()


def test_lattice_zero_extent_axis_and_ties():
    v, t = L.lattice(3000)
    info, extent = _check(v, t)
    assert info["leaf_triangles"] == 3000
    assert extent[2] == 0 and extent[0] > 1 and extent[1] > 1   # the z cells are all 0


def test_copies_are_in_triangle_order():
    v, t = L.copies(70)
    info, extent = _check(v, t)
    assert info["leaf_triangles"] == 70 and (extent == 0).all()


def test_scene_S(workdir):
    arr = S.base_arrays(workdir)
    info, _ = _check(arr["vertices"], arr["triangles"])
    assert info["always"] == 1 and info["never"] == 1 and info["leaf_triangles"] == 1640


def test_order_survives_a_refit_and_sah_has_one_too():
    v, t = L.soup(300, 7, 0.05, 0.05)
    with L.create(v, t) as sc, L.create(v, t, builder="sah") as sah:
        leaf, always = sc.bvh_order()
        assert sc.update_vertices(L.move(v)) == "refit"
        leaf2, always2 = sc.bvh_order()
        assert np.array_equal(leaf, leaf2) and np.array_equal(always, always2)   # a refit keeps the topology
        sl, sa = sah.bvh_order()
        assert np.array_equal(sa, always)                    # the always list is the builder's business in neither
        assert np.array_equal(np.sort(sl), np.sort(leaf))    # the same triangles, in the SAH builder's order


def test_order_argument_checks():
    import ctypes as C
    v, t = L.soup(40, 3, 0.1, 0.1)
    with L.create(v, t) as sc:
        info = sc.bvh_info()
        nl, na = info["leaf_triangles"], info["always"]
        assert nl > 0 and na > 0
        leaf, always = np.full(nl, 0xFFFFFFFF, np.uint32), np.full(na, 0xFFFFFFFF, np.uint32)
        a, b = C.c_int64(-1), C.c_int64(-1)
        fn = _capi.lib().rt_scene_bvh_order
        lp, ap = leaf.ctypes.data_as(C.c_void_p), always.ctypes.data_as(C.c_void_p)
        assert fn(None, lp, nl, C.byref(a), ap, na, C.byref(b)) == _capi.RT_E_ARG
        assert fn(sc.handle, None, nl, C.byref(a), ap, na, C.byref(b)) == _capi.RT_E_ARG
        assert fn(sc.handle, lp, nl, None, ap, na, C.byref(b)) == _capi.RT_E_ARG
        assert fn(sc.handle, lp, nl, C.byref(a), None, na, C.byref(b)) == _capi.RT_E_ARG
        assert fn(sc.handle, lp, nl, C.byref(a), ap, na, None) == _capi.RT_E_ARG
        # short buffers: the counts come back, nothing is copied
        assert fn(sc.handle, lp, nl - 1, C.byref(a), ap, na, C.byref(b)) == _capi.RT_E_ARG
        assert (a.value, b.value) == (nl, na) and (leaf == 0xFFFFFFFF).all() and (always == 0xFFFFFFFF).all()
        assert fn(sc.handle, lp, nl, C.byref(a), ap, na - 1, C.byref(b)) == _capi.RT_E_ARG
        assert (leaf == 0xFFFFFFFF).all() and (always == 0xFFFFFFFF).all()
        assert fn(sc.handle, lp, nl, C.byref(a), ap, na, C.byref(b)) == _capi.RT_OK
        want_leaf, want_always = sc.bvh_order()
        assert np.array_equal(leaf, want_leaf) and np.array_equal(always, want_always)


@pytest.mark.parametrize("name,depth", [("copies2500", 12), ("lattice3000", 13)])
def test_tie_scenes_build_without_fallback(name, depth):
    v, t = L.copies(2500) if name == "copies2500" else L.lattice(3000)
    with L.create(v, t) as sc:
        assert sc.bvh_info()["depth"] == depth
        assert sc.builder == ("lbvh", "lbvh")
