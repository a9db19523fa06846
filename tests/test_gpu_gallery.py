"""The kernels' shading arithmetic (shade_hit, fold_inlane / fold_chain, store_pixel, spec_powf, glibc_powf2)
over the material gallery of tests/_gallery.py, against the oracle with no tolerance.

The expected colours come from the oracle evaluating the specular power with the host build of the kernels'
own spec_pow.h (oracle.spec_pow("twin"); tests/test_gpu_device_math.py shows the device build gives its
bits), so every float is compared bit for bit; NaN compares as NaN, not by payload or sign (0 * inf is a
different NaN on x86 and on the GPU). tests/test_gallery.py shows, on the oracle alone, that the ray list
reaches every branch of shade() and refraction(), non-finite, negative and large colours, and that every
feature-flag set changes at least 50 colours.
"""
import numpy as np
import pytest
import torch

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi

import _gallery as G
from test_gpu_edge_rays import CHAIN_VARIANTS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STRIDES = (3, 4)
DEFAULT_VARIANT = CHAIN_VARIANTS[0]


def _ints(c):
    return [int(x) for x in c]


def _dev_rays(o, d, stride):
    if stride == 4:
        o = np.concatenate([o, np.full((len(o), 1), 123.0, np.float32)], axis=1)
        d = np.concatenate([d, np.full((len(d), 1), np.nan, np.float32)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(o)).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)


def _rp(flags=G.ALL, camera="default", max_lvl=G.MAX_LVL, lights=None, view=None, pf=1):
    return R.RenderParams(width=G.VIEW_W, height=G.VIEW_H, pf=pf, max_lvl=max_lvl, lights=G.LIGHTS if lights is None else lights,
                          flags=flags, camera_pos=G.CAMERAS[camera], corners=G.view_corners(view or "above"))


class Gallery:
    """One gallery file, its oracle, the list G, and the twin oracle's answers (computed once, never changed)."""

    def __init__(self, workdir, stem="gallery", scale=1.0, canopy="Top"):
        self.path = G.write_scene(workdir, stem, scale=scale, canopy=canopy)
        self.orc = O.OracleScene(self.path)
        self.o, self.d, self.tile, self.above = G.rays(scale=scale)
        self._list, self._frame = {}, {}

    def want_list(self, **kw):
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in self._list:
            with O.spec_pow("twin"):
                rgb, counts = G.trace_list(self.orc, G.params(**kw), self.o, self.d)
            rgb.setflags(write=False)
            self._list[key] = (rgb, _ints(counts))
        return self._list[key]

    def want_frame(self, **kw):
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in self._frame:
            with O.spec_pow("twin"):
                f32, u8, counts = self.orc.render(G.params(**kw))
            self._frame[key] = (f32, u8, _ints(counts))
        return self._frame[key]


@pytest.fixture(scope="module")
def gal(workdir, gpu_available):
    return Gallery(workdir)


def _same(got, want, what):
    assert G.same_bits(got, want), (what,) + G.first_difference(got, want)


def _list_all_entries(sc, gal, what, **kw):
    """perform_ray_tracing: the twin oracle's colours and counts; perform_ray_tracing_device, both strides: its bits."""
    want, counts = gal.want_list(**kw)
    P = _rp(**kw)
    rgb, c = sc.perform_ray_tracing(P, gal.o, gal.d)
    _same(rgb, want, what + ", host entry")
    assert _ints(c) == counts, (what, _ints(c), counts)
    for stride in STRIDES:
        drgb, dc = sc.perform_ray_tracing_device(P, *_dev_rays(gal.o, gal.d, stride), want_counts=True)
        _same(drgb.cpu().numpy(), want, f"{what}, device entry stride {stride}")
        assert _ints(dc) == counts, (what, stride)


def _set_variant(sc, variant):
    name, knobs = variant
    for k, v in knobs.items():
        sc.tune(k, v)
    sc.set_accel("brute_force" if name == "brute force" else "bvh")


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", list(G.CAMERAS))
@pytest.mark.parametrize("flagset", G.FLAG_SETS, ids=[n for n, _ in G.FLAG_SETS])
def test_ray_list_under_every_flag_set(gal, flagset, camera):
    """RT_ALL_FEATURES: every chain variant, stepwise (chain_from 255: k_shade and the frame-style fold) and
    in-lane (chain_from 0: k_chain and fold_inlane). The other sets: the default variant both ways."""
    name, flags = flagset
    with R.Scene.load(gal.path, device=0) as sc:
        for variant in (CHAIN_VARIANTS if flags == G.ALL else [DEFAULT_VARIANT]):
            _set_variant(sc, variant)
            for chain_from in (0, 255):
                sc.tune("chain_from", chain_from)
                _list_all_entries(sc, gal, f"{name}, camera {camera}, {variant[0]}, chain_from {chain_from}", flags=flags, camera=camera)


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flagset", [G.FLAG_SETS[0], G.FLAG_SETS[6]], ids=["all", "no_refraction"])
def test_debug_trace_of_every_eighth_ray(gal, flagset):
    name, flags = flagset
    assert flags in (G.ALL, G.ALL & ~G.REFRACTION)
    P, op = _rp(flags=flags), G.params(flags=flags)
    pick = np.arange(0, len(gal.o), 8)
    bounces = 0
    with R.Scene.load(gal.path, device=0) as sc:
        rgb_all, _ = sc.perform_ray_tracing(P, gal.o[pick], gal.d[pick])
        for j, i in enumerate(pick):
            with O.spec_pow("twin"):
                want, wrgb = gal.orc.debug_trace(op, gal.o[i], gal.d[i])
            got, rgb = sc.debug_trace(P, gal.o[i], gal.d[i])
            assert len(got) == len(want), (name, i)
            for k, (a, b) in enumerate(zip(got, want)):
                assert (a["triangle"], a["level"], a["shadowed"], a["lit"]) == (b["triangle"], b["level"], b["shadowed"], b["lit"]), (name, i, k)
                for f in ("origin", "dest") + (("hit",) if b["triangle"] >= 0 else ()):
                    assert G.same_bits(a[f], b[f]), (name, i, k, f, a[f], b[f])
            assert G.same_bits(rgb, wrgb) and G.same_bits(rgb, rgb_all[j]), (name, i)
            bounces += len(want)
    assert bounces >= 2 * len(pick)


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_lvl", [0, 1, 2])
def test_shallow_depths(gal, max_lvl):
    with R.Scene.load(gal.path, device=0) as sc:
        for chain_from in (0, 255):
            sc.tune("chain_from", chain_from)
            _list_all_entries(sc, gal, f"max_lvl {max_lvl}, chain_from {chain_from}", max_lvl=max_lvl)


def test_depth_12_between_two_mirrors(workdir, gpu_available):
    """The canopy takes the Gloss material (Ks 0.9 0.5 0.1), so chains bounce between it and the backdrop down
    to max_lvl 12: the in-lane records of steps past RT_LDS_RECORDS (3) go through chain_local."""
    deep = Gallery(workdir, "gallery_deep", canopy="Gloss")
    with O.spec_pow("twin"):
        _, lengths = G.coverage(deep.orc, G.params(max_lvl=12), deep.o, deep.d, max_lvl=12)
    assert (lengths >= 8).sum() >= 100 and lengths.max() == 13, np.bincount(lengths)
    with R.Scene.load(deep.path, device=0) as sc:
        for chain_from in (0, 255):
            sc.tune("chain_from", chain_from)
            _list_all_entries(sc, deep, f"max_lvl 12, chain_from {chain_from}", max_lvl=12)


# 4 -------------------------------------------------------------------------------------------------
def _frame_is_the_oracles(sc, gal, what, P, kw, launches=1, f32=True):
    wf32, wu8, wcounts = gal.want_frame(**kw)
    for i in range(launches):
        u8, gf32, c = sc.render(P, want_f32=f32)
        assert _ints(c) == wcounts, (what, i, _ints(c), wcounts)
        assert np.array_equal(u8, wu8), (what, i, "bytes", int((u8 != wu8).sum()), np.argwhere(u8 != wu8)[:4].tolist())
        if f32:
            _same(gf32, wf32, f"{what}, launch {i}, floats")


@pytest.mark.parametrize("flags", [G.ALL, G.ALL & ~G.SHADOWS], ids=["all", "no_shadows"])
@pytest.mark.parametrize("camera", list(G.CAMERAS))
@pytest.mark.parametrize("view", list(G.VIEW_Z0))
def test_frames(gal, view, camera, flags):
    """Floats, bytes (exactly: the clamp, the truncation and the NaN -> 0 rule of store_pixel) and counts of a
    frame, through rt_render_tile, the fused device frame, pf 2 (the average of sub-samples includes inf and
    NaN), the stealing kernel and the quad walk."""
    kw = dict(view=view, camera=camera, flags=flags)
    what = f"view {view}, camera {camera}, flags {flags:#x}"
    wf32, wu8, wcounts = gal.want_frame(**kw)
    # the picture is not empty (the oracle: 0.19 lit and 22 colours at the least, with shadows on and the camera below)
    assert (wf32 > 0).any(axis=2).mean() > 0.15 and len(np.unique(wu8.reshape(-1, 3), axis=0)) >= 20
    if flags != G.ALL and camera == "below":
        assert np.isnan(wf32).sum() >= 100 and (wf32 == 1).sum() >= 1000             # NsNeg's 0 * inf, and the clamp at 1
    with R.Scene.load(gal.path, device=0) as sc:
        P = _rp(**kw)
        _frame_is_the_oracles(sc, gal, what, P, kw)
        buf = torch.zeros(G.VIEW_H * G.VIEW_W * 3, dtype=torch.uint8, device=DEV)
        sc.tune("fuse_pixels", 1)
        c = sc.render_frame_device(P, 16, 16, buf.data_ptr(), buf.numel(), torch.cuda.current_stream(DEV).cuda_stream, want_counts=True)
        torch.cuda.synchronize(DEV)
        got = buf.cpu().numpy().reshape(G.VIEW_H, G.VIEW_W, 3)
        assert _ints(c) == wcounts and np.array_equal(got, wu8), (what, "device frame", int((got != wu8).sum()))
        kw2 = dict(kw, pf=2)
        _frame_is_the_oracles(sc, gal, what + ", pf 2", _rp(**kw2), kw2)
        # as test_frames_of_long_rays_through_every_chain_kernel sets them
        sc.tune("wave_steal", 0)
        sc.tune("chain_split", 0)
        sc.tune("steal_half", 0)
        sc.tune("steal_quarter", 0)
        _frame_is_the_oracles(sc, gal, what + ", plain walk", P, kw)
        sc.tune("wave_steal", 1)
        _frame_is_the_oracles(sc, gal, what + ", wave_steal", P, kw, launches=2)
        sc.tune("wave_steal", 0)
        sc.tune("steal_quarter", 4096)
        sc.tune("quad_walk", 1)
        _frame_is_the_oracles(sc, gal, what + ", quad_walk", P, kw, launches=4)


@pytest.mark.parametrize("flagset", G.FLAG_SETS[1:], ids=[n for n, _ in G.FLAG_SETS[1:]])
def test_frame_under_every_flag_set(gal, flagset):
    """A ray list's chain records go to memory and are folded by k_fold_rays; only a fused frame launch folds in
    the lane (fold_inlane, which re-derives each coefficient from the record's code). So the view "above" is
    rendered under every other flag set too, with the stealing kernel once."""
    name, flags = flagset
    kw = dict(view="above", flags=flags)
    with R.Scene.load(gal.path, device=0) as sc:
        _frame_is_the_oracles(sc, gal, name, _rp(**kw), kw)
        sc.tune("wave_steal", 1)
        _frame_is_the_oracles(sc, gal, name + ", wave_steal", _rp(**kw), kw)


# 5 -------------------------------------------------------------------------------------------------
def test_more_lights_than_the_inline_array(gal):
    """18 lights: the per-step kernels with kExtLights, which normalise the light position themselves instead
    of reading the host's p.lnorm."""
    lights = G.ring_lights()
    assert len(lights) == 18 and len(lights) > _capi.RT_MAX_LIGHTS
    with R.Scene.load(gal.path, device=0) as sc:
        _list_all_entries(sc, gal, "18 lights", lights=lights)
        kw = dict(view="above", lights=lights)
        _frame_is_the_oracles(sc, gal, "18 lights, view above", _rp(**kw), kw)


# 6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["lbvh", "cluster"])
def test_after_update_vertices(gal, workdir, builder):
    """The scene scaled by 2 about the origin through update_vertices: the device's refit normals and records
    then feed `check`, the acos threshold and the hit points. The reference is the scaled file's own oracle."""
    twice = Gallery(workdir, "gallery_x2", scale=2.0)
    with R.Scene.load(gal.path, device=0) as sc:
        v = sc.export()["vertices"]
        sc.set_builder(builder)
        assert sc.update_vertices(v, "rebuild") == "rebuilt_" + builder
        _list_all_entries(sc, gal, builder + ", rebuilt")
        assert sc.update_vertices((v * np.float32(2)).astype(np.float32)) in ("refit", "rebuilt_" + builder)
        assert np.array_equal(sc.export()["vertices"], twice.orc.export()["vertices"])
        _list_all_entries(sc, twice, builder + ", vertices x 2")
