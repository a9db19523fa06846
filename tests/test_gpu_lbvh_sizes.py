"""The GPU BVH builder (k_lbvh_*) and the refit (k_refit_*) at every internal size boundary.

tests/test_gpu_lbvh.py runs the kernels on 1,642 triangles and less, where every multi-workgroup path
takes its trivial branch. Each case here crosses one boundary (DESIGN.md "GPU BVH build" has the table of
constants and sizes): the device-built tree must equal the host statement bit for bit (digest: both node
arrays, the leaf order, the always list), validate as read back from the GPU, refit to the host's refit,
and rebuild to the same bytes in the same scratch. Four cases are also checked without any tree: queries
through the tree equal brute force over all triangles. Scenes are tests/_lbvh_scenes.py's.
"""
import functools

import numpy as np
import pytest

import raytracert_amd as R

import _lbvh_scenes as L

pytestmark = pytest.mark.gpu

SOUP = dict(always=0.03, never=0.03)
CASES = {
    # RT_BVH_MAX_LEAF = 2: the root is a leaf; the first emitted node; the first inner child
    **{"np%d" % n: functools.partial(L.soup_exact, n) for n in (2, 3, 4, 5)},
    # np - 1 radix nodes across a wave and across a block of 256
    **{"np%d" % n: functools.partial(L.soup_exact, n) for n in (64, 65, 256, 257, 258)},
    # kLbvhSortItems = 2048: under one, exactly one, two and three sort blocks, np < nt
    # 256 * sort_blocks > 1024 (k_lbvh_scan, two entries per lane): sort_blocks 5, 5, 6
    **{"soup%d" % n: functools.partial(L.soup, n, n, **SOUP) for n in (2047, 2048, 2049, 4097, 8193, 10240, 10241)},
    # equal codes across a sort block
    "copies2500": functools.partial(L.copies, 2500),
    "lattice3000": functools.partial(L.lattice, 3000),
    # more than 1024 blocks of 256 (k_lbvh_idscan, k_lbvh_bounds: two entries per lane)
    "soup262401": functools.partial(L.soup, 262401, 262401, always=0.002, never=0.002),
}
QUERY_CASES = ["soup2049", "soup10241", "lattice3000", "soup262401"]
ORIGIN = np.array([0.3, -0.2, 3.5], np.float32)
ORIGIN_MOVED = np.array([0.425, -0.35, 4.675], np.float32)   # ORIGIN under L.move


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, t = CASES[name]()
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def _host(name, builder="lbvh"):
    """The host statement of a case, computed once: digest, info and order of the tree of v, and the digest
    after the refit with move(v)."""
    v, t = _mesh(name)
    return _host_facts(v, t, builder)


def _host_facts(v, t, builder="lbvh"):
    with L.create(v, t, builder=builder) as h:
        facts = dict(digest=h.bvh_digest(), info=h.bvh_info(), order=h.bvh_order())
        assert h.builder == (builder, builder), "the host build fell back"
        assert h.update_vertices(L.move(v)) == "refit"
        facts["moved_digest"] = h.bvh_digest()
    return facts


def _core(v, t, want):
    with L.create(v, t, device=0) as sc:
        assert sc.bvh_digest() == want["digest"]
        assert sc.builder == ("lbvh", "lbvh"), "the device build fell back"
        assert sc.bvh_info() == want["info"]
        sc.bvh_validate()   # the arrays read back from the GPU
        assert sc.update_vertices(L.move(v)) == "refit"   # the device-made tri_slot, lvl2 and lvl4 tables
        assert sc.bvh_digest() == want["moved_digest"]
        sc.bvh_validate()
        assert sc.update_vertices(v, mode="rebuild") == "rebuilt_lbvh"   # a second build into the same scratch
        assert sc.builder == ("lbvh", "lbvh")
        assert sc.bvh_digest() == want["digest"]
        assert sc.bvh_info() == want["info"]


@pytest.mark.parametrize("name", list(CASES))
def test_build_refit_rebuild_equal_the_host_statement(name, gpu_available):
    v, t = _mesh(name)
    want = _host(name)
    info = want["info"]
    assert info["leaf_triangles"] + info["always"] + info["never"] == len(t)
    if name.startswith("np"):
        assert info["leaf_triangles"] == int(name[2:]) and info["always"] == 0 and info["never"] == 0
    if name.startswith("soup"):
        assert info["always"] > 0 and info["never"] > 0   # np < nt: the radix passes' n is the device's
    _core(v, t, want)


def test_indexed_grid_more_triangles_than_vertices(workdir, gpu_available):
    v, t = L.indexed_grid(workdir)
    assert len(t) > len(v) and len(t) > 2048   # k_lbvh_classify's grid is sized by nt
    _core(v, t, _host_facts(v, t))


def _rays(v, t, tree, origin, seed):
    """256 rays from `origin` at the centroids of randomly chosen tree triangles, and 32 that leave the
    scene's bounds behind them."""
    rng = np.random.default_rng(seed)
    pick = tree[rng.integers(0, len(tree), 256)]
    aimed = v[t[pick]].astype(np.float64).mean(axis=1)
    away = origin + np.concatenate([rng.uniform(-1, 1, (32, 2)), np.ones((32, 1))], axis=1)   # z grows: the scene is below
    assert origin[2] > v[:, 2].max()
    d = np.concatenate([aimed, away]).astype(np.float32)
    return np.tile(origin, (len(d), 1)).astype(np.float32), d


def _queries_equal_brute_force(sc, o, d):
    out = {}
    for width in (4, 2):
        sc.tune("bvh_width", width)
        out[width] = sc.intersect_mesh(o, d)
    sc.tune("bvh_width", 4)
    sc.set_accel("brute_force")
    idx, pts = sc.intersect_mesh(o, d)
    sc.set_accel("bvh")
    assert (idx[:256] >= 0).sum() >= 128, "the comparison must not pass on misses"
    assert (idx[256:] < 0).all()
    for width, (i, p) in out.items():
        assert np.array_equal(i, idx), width
        assert np.array_equal(p.view(np.uint32), pts.view(np.uint32)), width
    return idx, pts


@pytest.mark.parametrize("name", QUERY_CASES)
def test_queries_equal_brute_force(name, gpu_available):
    v, t = _mesh(name)
    want = _host(name)
    o, d = _rays(v, t, want["order"][0], ORIGIN, 11)
    with L.create(v, t, device=0) as sc:
        assert sc.bvh_digest() == want["digest"] and sc.builder == ("lbvh", "lbvh")
        _queries_equal_brute_force(sc, o, d)


@pytest.mark.parametrize("name", ["soup2049", "soup10241"])
def test_order_of_a_device_build(name, gpu_available):
    """rt_scene_bvh_order on the lazily read-back topology."""
    v, t = _mesh(name)
    leaf, always = _host(name)["order"]
    with L.create(v, t, device=0) as sc:
        got_leaf, got_always = sc.bvh_order()
        assert sc.builder == ("lbvh", "lbvh")
        assert np.array_equal(got_leaf, leaf) and np.array_equal(got_always, always)
        assert len(leaf) + len(always) + sc.bvh_info()["never"] == len(t)


def test_refit_of_a_host_built_tree_at_size(gpu_available):
    """A SAH device scene: the refit's tables are the host's (ensure_refit_topo), level groups of thousands
    of nodes."""
    v, t = _mesh("soup10241")
    want = _host("soup10241", "sah")
    moved = L.move(v)
    o, d = _rays(moved, t, want["order"][0], ORIGIN_MOVED, 12)
    with L.create(v, t, device=0, builder="sah") as sc:
        assert sc.bvh_digest() == want["digest"] and sc.builder == ("sah", "sah")
        assert sc.update_vertices(moved) == "refit"
        assert sc.bvh_digest() == want["moved_digest"]
        sc.bvh_validate()
        idx, pts = _queries_equal_brute_force(sc, o, d)
    with L.create(moved, t, device=0, builder="sah") as fresh:   # and a scene created from the moved vertices
        fi, fp = fresh.intersect_mesh(o, d)
        assert np.array_equal(fi, idx) and np.array_equal(fp.view(np.uint32), pts.view(np.uint32))
