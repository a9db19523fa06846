"""The agglomerative GPU builder (k_cluster_*) at every internal size boundary.

tests/test_gpu_cluster.py runs the kernels on 1,642 triangles and less. Each case here crosses one boundary
(DESIGN.md "GPU BVH build: RT_BUILD_CLUSTER" has the table): the device-built tree must equal the host
statement bit for bit (digest: both node arrays, the leaf order, the always list), take the same number of
clustering iterations, validate as read back from the GPU, refit to the host's refit, and rebuild to the
same bytes in the same scratch. Some cases are also checked without any tree: queries through both trees
equal brute force over all triangles. The sizes come from rt_scene_build_info's window radius r and tail
threshold T, not from literals. Scenes are tests/_lbvh_scenes.py's.
"""
import functools

import numpy as np
import pytest

import raytracert_amd as R

import _lbvh_scenes as L

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _constants():
    """(r, T) from rt_scene_build_info, read when the first test runs (collection loads nothing)."""
    v, t = L.soup_exact(3)
    with L.create(v, t, builder="cluster") as h:
        bi = h.build_info()
    assert bi["radius"] >= 1 and bi["tail"] >= 1
    return bi["radius"], bi["tail"]


BLOCK = 256   # one workgroup's clusters; its LDS stage holds BLOCK + 2 r boxes
SCAN_ENTRIES = 1024 * BLOCK   # k_cluster_scan: one block count per lane up to this many clusters
# np of each case, as a function of (r, T): a constant that moves takes its sizes with it
NP = {
    # RT_BVH_MAX_LEAF = 2: wrapped root, first node, first inner children
    "np2": lambda r, T: 2, "np3": lambda r, T: 3, "np4": lambda r, T: 4, "np5": lambda r, T: 5,
    # the window reaches past both ends of the array / past one end / fits
    "np_r": lambda r, T: r, "np_r+1": lambda r, T: r + 1, "np_2r": lambda r, T: 2 * r, "np_2r+1": lambda r, T: 2 * r + 1,
    # a wave
    "np64": lambda r, T: 64, "np65": lambda r, T: 65,
    # a block and its halo
    "np255": lambda r, T: BLOCK - 1, "np256": lambda r, T: BLOCK, "np257": lambda r, T: BLOCK + 1,
    "np_256+r": lambda r, T: BLOCK + r, "np_256+r+1": lambda r, T: BLOCK + r + 1, "np512": lambda r, T: 2 * BLOCK, "np513": lambda r, T: 2 * BLOCK + 1,
    # the single-workgroup tail
    "np_T-1": lambda r, T: T - 1, "np_T": lambda r, T: T, "np_T+1": lambda r, T: T + 1, "np_2T+1": lambda r, T: 2 * T + 1,
    # kLbvhSortItems = 2048
    "np2047": lambda r, T: 2047, "np2048": lambda r, T: 2048, "np2049": lambda r, T: 2049, "np4097": lambda r, T: 4097,
}
BIG = "soup264000"   # np = 262,918 tree triangles: more than 1,024 blocks of 256 clusters
CASES = {
    **{name: None for name in NP},
    # equal boxes: the key's XOR part decides everything
    "copies2500": functools.partial(L.copies, 2500),
    "lattice3000": functools.partial(L.lattice, 3000),
    # np < nt: the cluster count starts from the device's np
    "soup3000": functools.partial(L.soup, 3000, 3000, always=0.03, never=0.03),
    # np > 1024 * 256 (k_cluster_scan: two block counts per lane in the first iterations); the always and never
    # fractions take about 1,080 triangles away, so nt is chosen well above the bound
    BIG: functools.partial(L.soup, 264000, 264000, always=0.002, never=0.002),
}
QUERY_CASES = ["np_2r+1", "np257", "np_T+1", "lattice3000", BIG]
ORIGIN = np.array([0.3, -0.2, 3.5], np.float32)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, t = L.soup_exact(NP[name](*_constants())) if name in NP else CASES[name]()
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def _host_facts(v, t):
    with L.create(v, t, builder="cluster") as h:
        facts = dict(digest=h.bvh_digest(), info=h.bvh_info(), order=h.bvh_order(), build=h.build_info())
        assert h.builder == ("cluster", "cluster"), "the host build fell back"
        assert h.update_vertices(L.move(v)) == "refit"
        facts["moved_digest"] = h.bvh_digest()
    return facts


@functools.lru_cache(maxsize=None)
def _host(name):
    """The host statement of a case, computed once."""
    return _host_facts(*_mesh(name))


def _core(v, t, want):
    with L.create(v, t, device=0, builder="cluster") as sc:
        assert sc.bvh_digest() == want["digest"]
        assert sc.builder == ("cluster", "cluster"), "the device build fell back"
        assert sc.bvh_info() == want["info"]
        assert sc.build_info() == want["build"]   # (the iteration count and the cost among them)
        sc.bvh_validate()   # the arrays read back from the GPU
        assert sc.update_vertices(L.move(v)) == "refit"   # the device-made tri_slot, lvl2 and lvl4 tables
        assert sc.bvh_digest() == want["moved_digest"]
        sc.bvh_validate()
        assert sc.update_vertices(v, mode="rebuild") == "rebuilt_cluster"   # a second build into the same scratch
        assert sc.builder == ("cluster", "cluster")
        assert sc.bvh_digest() == want["digest"]
        assert sc.bvh_info() == want["info"] and sc.build_info() == want["build"]


@pytest.mark.parametrize("name", list(CASES))
def test_build_refit_rebuild_equal_the_host_statement(name, gpu_available):
    v, t = _mesh(name)
    want = _host(name)
    info = want["info"]
    assert info["leaf_triangles"] + info["always"] + info["never"] == len(t)
    if name in NP:
        n = NP[name](*_constants())
        assert info["leaf_triangles"] == n and info["always"] == 0 and info["never"] == 0
        assert (want["build"]["iterations"] > 0) == (n > 2)
    if name.startswith("soup"):
        assert info["always"] > 0 and info["never"] > 0
    if name == BIG:
        assert info["leaf_triangles"] > SCAN_ENTRIES   # the cluster count, not nt, sizes k_cluster_scan
    if name == "copies2500":
        assert want["build"]["iterations"] == 12   # the halvings 2500 -> 1
    _core(v, t, want)


def test_indexed_grid_more_triangles_than_vertices(workdir, gpu_available):
    v, t = L.indexed_grid(workdir)
    assert len(t) > len(v) and len(t) > 2048
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


@pytest.mark.parametrize("name", QUERY_CASES)
def test_queries_equal_brute_force(name, gpu_available):
    v, t = _mesh(name)
    want = _host(name)
    o, d = _rays(v, t, want["order"][0], ORIGIN, 11)
    with L.create(v, t, device=0, builder="cluster") as sc:
        assert sc.bvh_digest() == want["digest"] and sc.builder == ("cluster", "cluster")
        out = {}
        for width in (4, 2):
            sc.tune("bvh_width", width)
            out[width] = sc.intersect_mesh(o, d)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        idx, pts = sc.intersect_mesh(o, d)
        assert (idx[:256] >= 0).sum() >= 128, "the comparison must not pass on misses"
        assert (idx[256:] < 0).all()
        for width, (i, p) in out.items():
            assert np.array_equal(i, idx), width
            assert np.array_equal(p.view(np.uint32), pts.view(np.uint32)), width


@pytest.mark.parametrize("every", [0, 3, 8])
def test_blind_and_read_back_builds_are_the_same_tree(every, monkeypatch, gpu_available):
    """The host either queues the whole iteration budget blind (0) or reads the cluster count back after
    every N iterations and stops queueing at the tail's size; the same iterations run, so the trees are
    the same. 3: the hand-over to the tail falls on either entry of the ping-pong arrays."""
    monkeypatch.setenv("RTAMD_CLUSTER_READBACK", str(every))
    for name in ("np_T", "np_T+1", "np_2T+1", "np4097", "lattice3000", "soup3000"):
        v, t = _mesh(name)
        want = _host(name)
        with L.create(v, t, device=0, builder="cluster") as sc:
            assert sc.bvh_digest() == want["digest"], name
            assert sc.builder == ("cluster", "cluster") and sc.build_info() == want["build"], name
            assert sc.update_vertices(L.move(v)) == "refit" and sc.bvh_digest() == want["moved_digest"], name
            assert sc.update_vertices(v, mode="rebuild") == "rebuilt_cluster" and sc.bvh_digest() == want["digest"], name
