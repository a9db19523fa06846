"""Every traversal against the oracle on rays the slab code and the distance cull special-case: direction
components of exactly +0 / -0, zero-length, very long (dot(dir, dir) overflows), very short, far origins (the
pad exceeds the scene), origins on box planes, rays through vertices and along edges, non-finite components.
Scene, ray classes and what the oracle alone says about them: tests/_edge_rays.py, tests/test_edge_rays.py.

Index and hit-point bits of all rays are compared (any NaN equal to any NaN), through rt_intersect_mesh and
rt_intersect_mesh_device (strides 3 and 4), for brute force, the four-wide walk, the binary walk and the three
builders; occlusion by both walks; the device queries' own stack overflow area (lds_stack 1); the scene
scaled by 2^21 (scene_m1 >= 1e6: the binary tree by default) and by 2^10; the chain kernels over ray lists; frames whose
every primary ray is long, which is how the stealing and the quad walk meet such rays (ray lists are not
fused launches; launch_chain).

On the kernels before the per-ray cull switch (ray4_setup's inv_dlen, bvh_query's R.dlen), for |dir| above
2^63 (classes B): the binary walk culled every child (no hit beyond the always list), the four-wide walks
kept the first hit found (tcull 0). On the scaled scenes the longest rays make n.dir overflow, where the
reference accepts triangles by the origin's projection alone: both walks missed those until such rays were made
to meet every triangle (ndir_may_overflow). DESIGN.md section 7 records the cases that failed.
"""
import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R

import _edge_rays as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32_TOL = 2e-6                 # the suite's float RGB tolerance (tests/test_gpu_parity.py)
STRIDES = (3, 4)
IDX_SENTINEL = -7
NAN_SENTINEL = 0x7FC0DEAD      # a NaN bit pattern no kernel computes
LIGHTS = [[0.5, 1.0, 4.0]]
MIN_HITS = {"A": 100, "B": 3 * 200, "C": 2 * 200, "D": 5 * 200, "E": 0, "F": 3 * 200, "G": 4 * 32, "H": 0}
NO_HITS = ("C_1e-6", "E", "F_1e30", "H")


def _np(t):
    return t.cpu().numpy()


def _dev_rays(o, d, stride):
    """The rays as CUDA tensors in either layout; the padded layout's w holds values that must not matter."""
    if stride == 4:
        o = np.concatenate([o, np.full((len(o), 1), 123.0, np.float32)], axis=1)
        d = np.concatenate([d, np.full((len(d), 1), np.nan, np.float32)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(o)).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)


class Case:
    """One scene file, its oracle, and the oracle's answers per ray class (computed once, never changed)."""

    def __init__(self, workdir, stem, transparent=False, scale=1.0):
        self.path = E.write_scene(workdir, stem, transparent=transparent, scale=scale)
        self.orc = O.OracleScene(self.path)
        self.scale = scale
        self._rays, self._traced = {}, {}

    def rays(self, letter):
        if letter not in self._rays:
            o, d, where = E.class_rays(letter, self.scale)
            want = E.oracle_answers(self.orc, o, d)
            for a in want.values():
                a.setflags(write=False)
            hit = want["index"] >= 0
            assert hit.sum() >= MIN_HITS[letter]          # no case passes empty (tests/test_edge_rays.py)
            for name, s in where.items():
                assert (name in NO_HITS) == (not hit[s].any()) or self.scale != 1.0, name
            self._rays[letter] = (o, d, where, want)
        return self._rays[letter]

    def traced(self, letter, params):
        if letter not in self._traced:
            o, d, _, _ = self.rays(letter)
            rgb = np.array([self.orc.trace(params, o[i], d[i])[0] for i in range(len(o))], np.float32)
            rgb.setflags(write=False)
            self._traced[letter] = rgb
        return self._traced[letter]


@pytest.fixture(scope="module")
def plain(workdir, gpu_available):
    return Case(workdir, "shingles")


@pytest.fixture(scope="module")
def glassy(workdir, gpu_available):
    return Case(workdir, "shingles_tr", transparent=True)


@pytest.fixture(scope="module")
def big(workdir, gpu_available):
    return Case(workdir, "shingles_big", scale=E.BIG)


@pytest.fixture(scope="module")
def mid(workdir, gpu_available):
    return Case(workdir, "shingles_mid", scale=E.MID)


def _check_closest(idx, pts, want, what):
    idx, pts = np.asarray(idx), np.asarray(pts, np.float32)
    bad = np.flatnonzero(idx != want["index"])
    assert bad.size == 0, f"{what}: {bad.size} indices differ, first ray {bad[:5]}: {idx[bad[:5]]} for {want['index'][bad[:5]]}"
    assert E.same_bits(pts, want["point"]), f"{what}: hit points differ"


def _closest_all_entries(sc, o, d, want, what):
    """rt_intersect_mesh and rt_intersect_mesh_device in both layouts, all rays."""
    hidx, hpts = sc.intersect_mesh(o, d)
    _check_closest(hidx, hpts, want, what + ", host entry")
    for stride in STRIDES:
        do, dd = _dev_rays(o, d, stride)
        idx, pts = sc.intersect_mesh_device(do, dd)
        _check_closest(_np(idx), _np(pts), want, f"{what}, device entry stride {stride}")


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", list("ABCDEFGH"))
def test_closest_hit_of_every_traversal_is_the_oracles(plain, letter):
    o, d, _, want = plain.rays(letter)
    with R.Scene.load(plain.path, device=0) as sc:
        assert sc.accel() == "bvh" and sc.bvh_info()["nodes4"] > 21      # more than the breadth-first top
        _closest_all_entries(sc, o, d, want, "four-wide")
        sc.tune("bvh_width", 2)
        _closest_all_entries(sc, o, d, want, "binary")
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        _closest_all_entries(sc, o, d, want, "brute force")
        sc.set_accel("bvh")
        v = sc.export()["vertices"]
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(v, "rebuild") == "rebuilt_" + builder
            for width in (4, 2):
                sc.tune("bvh_width", width)
                _closest_all_entries(sc, o, d, want, f"{builder} width {width}")


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", list("ABCDEFGH"))
def test_occlusion_by_both_walks(plain, glassy, letter):
    o, d, _, opaque = plain.rays(letter)
    _, _, _, want = glassy.rays(letter)
    assert np.array_equal(want["index"], opaque["index"])       # the same geometry: only a material differs
    assert not opaque["transparent_closest"].any()
    if MIN_HITS[letter]:
        assert want["transparent_closest"].sum() >= 30 and want["blocked"].sum() >= 30
    # a transparent material in use: the closest-hit walk, the verdict from the closest hit's material
    with R.Scene.load(glassy.path, device=0) as sc:
        for what, width, accel in (("four-wide", 4, "bvh"), ("binary", 2, "bvh"), ("brute force", 4, "brute_force")):
            sc.tune("bvh_width", width)
            sc.set_accel(accel)
            for stride in STRIDES:
                blk = _np(sc.occluded_device(*_dev_rays(o, d, stride)))
                assert np.array_equal(blk, want["blocked"]), (what, stride, np.flatnonzero(blk != want["blocked"])[:8])
            _closest_all_entries(sc, o, d, want, "transparent twin, " + what)
    # every material opaque: the any-hit walk, blocked = the oracle hit something
    any_hit = (opaque["index"] >= 0).astype(np.uint8)
    with R.Scene.load(plain.path, device=0) as sc:
        for what, width, accel in (("four-wide", 4, "bvh"), ("binary", 2, "bvh"), ("brute force", 4, "brute_force")):
            sc.tune("bvh_width", width)
            sc.set_accel(accel)
            for stride in STRIDES:
                blk = _np(sc.occluded_device(*_dev_rays(o, d, stride)))
                assert np.array_equal(blk, any_hit), (what, stride, np.flatnonzero(blk != any_hit)[:8])


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", list("ABDF"))
def test_device_query_stack_overflow_area(plain, glassy, letter):
    """lds_stack 1: all but one entry of every lane's traversal stack lies in the device queries' own
    overflow area (ensure_stack_ovf: area index kMaxPipes, stack_entries - 1 rows of grid x block lanes;
    launch_query's grid is at most bvh_grid blocks, and a walk holds at most 3 entries per four-wide
    level, 1 per binary level, whatever the floats are). Three copies of the class: more than one block, with
    far origins (every box wanted: the deepest stacks) next to each other in every wave."""
    o, d, _, want = glassy.rays(letter)
    reps = 3
    o3, d3 = np.tile(o, (reps, 1)), np.tile(d, (reps, 1))
    want3 = {k: np.tile(a, (reps,) + (1,) * (a.ndim - 1)) for k, a in want.items()}
    assert len(o3) > 2 * 256
    for case, blocked in ((glassy, want3["blocked"]), (plain, (want3["index"] >= 0).astype(np.uint8))):
        with R.Scene.load(case.path, device=0) as sc:
            info = sc.bvh_info()
            assert 3 * info["depth4"] > 4 and info["depth"] > 4      # stacks deeper than the LDS part
            sc.tune("lds_stack", 1)
            for width in (4, 2):
                sc.tune("bvh_width", width)
                _closest_all_entries(sc, o3, d3, want3, f"lds_stack 1 width {width}")
                blk = _np(sc.occluded_device(*_dev_rays(o3, d3, 3)))
                assert np.array_equal(blk, blocked), (width, np.flatnonzero(blk != blocked)[:8])
            sc.tune("bvh_grid", 2)          # fewer blocks than the rays need: a grid-stride walk over the same area
            sc.tune("bvh_width", 4)
            _closest_all_entries(sc, o3, d3, want3, "lds_stack 1, bvh_grid 2")


# 4 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["big", "mid"])
@pytest.mark.parametrize("letter", list("ABD"))
def test_scaled_scenes(big, mid, size, letter):
    """Exact scaling of the scene and the rays by 2^21 (scene_m1 >= 1e6, so the binary tree walks whatever
    bvh_width says) and by 2^10 (the four-wide walk). The scaled file's own oracle is the reference: |n.dir| <
    1e-5 is not scale-free, and for the long rays n.dir overflows (2^21: every scale of class B; 2^10: 1e30),
    where the reference takes I = o and accepts triangles by the origin's projection alone, at distance 0: the
    walks must then meet every triangle (ndir_may_overflow in rt_kernels.hip)."""
    case = big if size == "big" else mid
    o, d, where, want = case.rays(letter)
    for name, s in where.items():
        assert (want["index"][s] >= 0).sum() >= (100 if letter == "A" else 200), name
    if letter == "B":
        s = where["B_1e30"]
        assert ((want["point"][s] == o[s]).all(axis=1) & (want["index"][s] >= 0)).sum() >= 200     # the overflow case
    with R.Scene.load(case.path, device=0) as sc:
        assert (np.abs(sc.export()["vertices"]).sum(axis=1).max() >= 1e6) == (size == "big")
        _closest_all_entries(sc, o, d, want, "scaled, default walk")
        sc.tune("bvh_width", 2)
        _closest_all_entries(sc, o, d, want, "scaled, width 2")
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        _closest_all_entries(sc, o, d, want, "scaled, brute force")
        blk_brute = _np(sc.occluded_device(*_dev_rays(o, d, 3)))
        sc.set_accel("bvh")
        blk = _np(sc.occluded_device(*_dev_rays(o, d, 3)))
        assert np.array_equal(blk, blk_brute) and np.array_equal(blk, (want["index"] >= 0).astype(np.uint8))
        v = sc.export()["vertices"]
        for builder in ("lbvh", "cluster"):
            sc.set_builder(builder)
            assert sc.update_vertices(v, "rebuild") == "rebuilt_" + builder
            _closest_all_entries(sc, o, d, want, "scaled, " + builder)


# 5 -------------------------------------------------------------------------------------------------
CHAIN_VARIANTS = [("plain", {"wave_steal": 0}), ("wave_steal", {"wave_steal": 1}), ("quad_walk", {"wave_steal": 0, "quad_walk": 1}),
                  ("binary", {"wave_steal": 0, "quad_walk": 0, "bvh_width": 2}), ("brute force", {"bvh_width": 4})]


@pytest.mark.parametrize("which", ["plain", "glassy"])
@pytest.mark.parametrize("letter", list("ABDFH"))
def test_chain_kernels_over_ray_lists(plain, glassy, which, letter):
    """performRayTracing of the class's rays, depth 2, one light, shadows on (any-hit shadow walks on the
    opaque scene, closest-hit ones and refraction on its transparent twin): the same bits from every
    variant and from the device entry, and the oracle's colours within the suite's tolerance (class H:
    among the GPU variants only)."""
    case = plain if which == "plain" else glassy
    o, d, _, want = case.rays(letter)
    P = R.RenderParams(width=64, height=64, pf=1, max_lvl=2, lights=LIGHTS)
    first = None
    with R.Scene.load(case.path, device=0) as sc:
        for name, knobs in CHAIN_VARIANTS:
            for k, v in knobs.items():
                sc.tune(k, v)
            sc.set_accel("brute_force" if name == "brute force" else "bvh")
            rgb, counts = sc.perform_ray_tracing(P, o, d)
            if first is None:
                first = (rgb, [int(c) for c in counts])
            assert E.same_bits(rgb, first[0]) and [int(c) for c in counts] == first[1], name
            for stride in STRIDES:
                drgb = sc.perform_ray_tracing_device(P, *_dev_rays(o, d, stride))
                assert E.same_bits(_np(drgb), first[0]), (name, stride)
    rgb = first[0]
    assert first[1][0] == len(o)
    if letter == "H":
        assert (want["index"] < 0).all()
        return
    orgb = case.traced(letter, O.make_params(64, 64, pf=1, max_lvl=2, lights=LIGHTS))
    assert np.isfinite(orgb).all() and len(np.unique(orgb.view(np.uint32), axis=0)) >= 20      # (the oracle: 25 and more)
    err = np.abs(rgb - orgb)
    assert np.isfinite(rgb).all() and err.max() <= F32_TOL, (float(err.max()), int((err > F32_TOL).any(axis=1).sum()))


# 6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("letter", list("BDF"))
def test_prefix_counts_put_edge_rays_in_the_last_partial_wave(glassy, letter, width, stride):
    o, d, _, want = glassy.rays(letter)
    cap = len(o) + 8
    with R.Scene.load(glassy.path, device=0) as sc:
        sc.tune("bvh_width", width)
        for n in E.PREFIXES + (len(o),):
            assert (want["index"][:n] >= 0).any()
            do, dd = _dev_rays(o[:n], d[:n], stride)
            idx = torch.full((cap,), IDX_SENTINEL, dtype=torch.int32, device=DEV)
            pts = torch.full((cap, 3), NAN_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            sc.intersect_mesh_device(do, dd, out=(idx, pts))
            blk = _np(sc.occluded_device(do, dd))
            idx, pb = _np(idx), _np(pts).view(np.uint32)
            assert np.array_equal(idx[:n], want["index"][:n]) and E.same_bits(_np(pts)[:n], want["point"][:n]), n
            assert (idx[n:] == IDX_SENTINEL).all() and (pb[n:] == NAN_SENTINEL).all(), n
            assert np.array_equal(blk, want["blocked"][:n]), n
            # the same prefix of the whole arrays by a device count
            fo, fd = _dev_rays(o, d, stride)
            cidx, cpts = sc.intersect_mesh_device(fo, fd, count=torch.tensor([n], dtype=torch.int32, device=DEV))
            assert np.array_equal(_np(cidx)[:n], want["index"][:n]) and (_np(cidx)[n:] == -1).all(), n
            assert E.same_bits(_np(cpts)[:n], want["point"][:n]), n


# 7 -------------------------------------------------------------------------------------------------
def _long_view(w, h, s):
    """The default view with every primary ray stretched by s: dest corner = origin corner + (dest - origin) s."""
    cs = R.default_corners(w, h).copy()
    cs[1::2] = (cs[0::2] + (cs[1::2] - cs[0::2]) * np.float32(s)).astype(np.float32)
    return cs


@pytest.mark.parametrize("which", ["plain", "glassy"])
def test_frames_of_long_rays_through_every_chain_kernel(plain, glassy, which):
    """Frames whose every primary ray has dot(dir, dir) = inf (corners stretched by 1e20): fused launches, so
    wave_steal 1 runs bvh4_query_steal and quad_walk 1 (with a quarter tier, from the second frame on) runs
    bvh4_query_quad on them. Bytes, floats and ray counts are the plain walk's on every launch, the binary
    walk's and brute force's; the floats are the oracle's within the suite's tolerance, and the unstretched
    view's hits (the picture is not empty)."""
    case = plain if which == "plain" else glassy
    W, H = 160, 90
    cs = _long_view(W, H, 1e20)
    P = R.RenderParams(width=W, height=H, pf=1, max_lvl=2, lights=LIGHTS, corners=cs)
    of32, ou8, ocounts = case.orc.render(O.make_params(W, H, pf=1, max_lvl=2, lights=LIGHTS, corners=cs))
    lit = (of32 > 0).any(axis=2)
    assert lit.mean() > 0.1 and len(np.unique(ou8.reshape(-1, 3), axis=0)) > 50      # (measured: 0.16 / 0.19, 94 / 114)
    with R.Scene.load(case.path, device=0) as sc:
        sc.tune("wave_steal", 0)
        sc.tune("chain_split", 0)
        sc.tune("steal_half", 0)
        sc.tune("steal_quarter", 0)
        ref, reff, refc = sc.render(P, want_f32=True)
        assert [int(c) for c in refc] == [int(c) for c in ocounts]
        err = np.abs(reff - of32)
        assert err.max() <= F32_TOL, ("plain walk against the oracle", float(err.max()), int((err > F32_TOL).any(axis=2).sum()))
        assert int(np.abs(ref.astype(np.int16) - ou8.astype(np.int16)).max()) <= 1

        def same(what, launches):
            for i in range(launches):
                u8, f32, c = sc.render(P, want_f32=True)
                assert [int(x) for x in c] == [int(x) for x in refc], (what, i)
                assert np.array_equal(u8, ref) and np.array_equal(f32.view(np.uint32), reff.view(np.uint32)), (what, i)

        sc.tune("wave_steal", 1)
        same("wave_steal", 2)
        sc.tune("wave_steal", 0)
        sc.tune("steal_quarter", 4096)
        sc.tune("quad_walk", 1)
        same("quad_walk", 4)
        sc.tune("quad_walk", 0)
        sc.tune("steal_quarter", 0)
        sc.tune("bvh_width", 2)
        same("binary", 1)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        same("brute force", 1)
