"""RT_TUNE_DARK_LIGHTS: the chain launch walks no shadow ray to a light that cannot reach a hit
(raytracert_amd/csrc/dark_lights.h), and every byte stays the oracle's.

Scenes F3 and F4 (F4: a transparent material, so the closest-hit shadow instantiation runs) at 96 x 54, pf 1 and
3, depth 3, under the light sets of tests/_dark_lights.py, whose preconditions are checked here on the CPU from
the oracle's hits and the rule restated in numpy: front lights (no primary hit dark, some secondary ones),
a light behind the scene with the eye beside it (nearly every primary hit dark), the same without the specular
term (one normalisation per light), three lights with the dark one first, in the middle and last, and a turned
view with two opposite lights (V + L nearly cancels on some hits).

The knob: 0 every walk, 1 (the default) the rule from a chain's second step on, 2 at every step (the light sets
whose primary hits are dark need 2). For each set: the bytes, the floats and the ray counts are the oracle's
with the knob at 2, 1 and 0; the per-sample colours (out_mode 2) are the same bits under all three and equal
the oracle's trace() of the sample's ray, at pf 1 for every sample and at pf 3 for every seventh (7 and 9 are
coprime, so every sub-sample offset is met; all 46,656 from Python would take several seconds);
rt_debug_trace equals ora_debug_trace on 64 pixels that include dark hits. The shadow walks' node visits fall
where a light is dark and stay where none is. The per-lane path, the split tiers with and without shadow
helpers, the stealing kernel, the quad walk and the multi-frame launch each give the oracle's frame. A material
with Ks = inf or Ns = 0 switches the rule off."""
import os

import numpy as np
import pytest

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _dark_lights as D

pytestmark = pytest.mark.gpu

F32 = np.float32
SCENES = ["F3", "F4"]


def _ints(c):
    return [int(x) for x in c]


def _same_bits(a, b, what):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _rp(case, pf, max_lvl=D.MAX_LVL):
    lights, corners, cam, flags = D.params(case)
    return R.RenderParams(width=D.W, height=D.H, pf=pf, max_lvl=max_lvl, lights=lights, flags=flags, camera_pos=cam, corners=corners)


def _op(case, pf, max_lvl=D.MAX_LVL):
    lights, corners, cam, flags = D.params(case)
    return O.make_params(D.W, D.H, pf, max_lvl, lights=lights, flags=flags, camera_pos=cam, corners=corners)


class Fixture:
    def __init__(self, name, workdir, mtl_edit=None, stem=None):
        self.path = scenes.write_sphere_grid(getattr(scenes, name), workdir, stem or ("dark_" + name.lower()))
        if mtl_edit:
            mtl = os.path.splitext(self.path)[0] + ".mtl"
            with open(mtl) as f:
                text = f.read()
            assert mtl_edit[0] in text
            with open(mtl, "w", newline="\n") as f:
                f.write(text.replace(*mtl_edit))
        self.orc = O.OracleScene(self.path)
        self.normals = self.orc.export()["normals"].astype(F32)
        self._want, self._hits = {}, {}

    def want(self, case, pf, max_lvl=D.MAX_LVL):
        """The oracle's (floats, bytes, counts), with the kernels' specular powf (its host twin): made once."""
        k = (case, pf, max_lvl)
        if k not in self._want:
            with O.spec_pow("twin"):
                f32, u8, counts = self.orc.render(_op(case, pf, max_lvl))
            self._want[k] = (f32, u8, _ints(counts))
        return self._want[k]

    def hits(self, case):
        if case not in self._hits:
            self._hits[case] = D.hits(self.orc, case)
        return self._hits[case]

    def candidates(self, case):
        """Per light: the dark-candidate hits of the case's pf 1 chains (rows of hits()), and which of them
        lie on faces whose normal the light's normalisations move."""
        lights, _, cam, flags = D.params(case)
        h = self.hits(case)
        tri, P = h[:, 2].astype(int), h[:, 3:6].astype(F32)
        spec = bool(flags & D.SPECULAR)
        stable = D.fixed_point(self.normals, 2 if spec else 1)[tri]
        return h, [D.candidates(self.normals[tri], P, l, cam, spec) for l in lights], stable


@pytest.fixture(scope="module", params=SCENES)
def fx(request, workdir):
    return Fixture(request.param, workdir)


@pytest.fixture(scope="module")
def dev(fx, gpu_available):
    with R.Scene.load(fx.path, device=0) as sc:
        sc.tune("wave_steal", 0)
        yield sc


def test_preconditions(fx):
    """The light sets do what they are for (CPU only: the oracle's hits and the rule in numpy)."""
    h, cand, stable = fx.candidates("front")
    prim = h[:, 1] == 0
    assert not any((c & prim).any() for c in cand) and sum(int((c & ~prim & stable).sum()) for c in cand) >= 10
    for case in ("behind", "behind_diffuse"):
        h, cand, stable = fx.candidates(case)
        prim = h[:, 1] == 0
        assert (cand[0] & prim & stable).sum() > 0.9 * prim.sum(), case
        # ... and the reference finds some of them lit: there it makes the normalisations the rule reasons about
        assert (cand[0] & stable & (h[:, 6].astype(int) & 1 == 0)).sum() >= 50, case
    for case, at in (("dark_first", 0), ("dark_middle", 1), ("dark_last", 2)):
        h, cand, stable = fx.candidates(case)
        prim = h[:, 1] == 0
        assert (cand[at] & stable).sum() > 0.9 * prim.sum()
        # the other two light most primary hits: the normal meets unshadowed lights before and after the dark one
        lit = [(prim & ~cand[k] & ((h[:, 6].astype(int) >> k) & 1 == 0)).sum() for k in range(3) if k != at]
        assert min(lit) > 0.5 * prim.sum(), lit
    # the turned view: hits where the unit view and light vectors nearly cancel, and dark hits beside them
    h, cand, stable = fx.candidates("turned")
    lights, _, cam, _ = D.params("turned")
    P = h[:, 3:6].astype(F32)
    V, L = D.normalize(np.asarray(cam, F32)[None, :] - P), D.normalize(np.asarray(lights[1], F32)[None, :] - P)
    assert (np.linalg.norm(V + L, axis=1) < 0.05).sum() >= 5 and np.linalg.norm(V + L, axis=1).min() < 1e-3
    assert sum(int((c & stable).sum()) for c in cand) >= 10
    # faces whose normal is not a fixed point exist, and dark candidates land on them: the fixed-point test decides
    assert 0.05 < (~D.fixed_point(fx.normals, 2)).mean() < 0.5
    unstable = 0
    for case in D.CASES:
        _, cand, stable = fx.candidates(case)
        unstable += sum(int((c & ~stable).sum()) for c in cand)
    assert unstable >= 50, unstable
    # ... and the fixed-point test decides bytes: some of those candidates the reference finds lit (it then moves
    # the normal, which the rule must not skip) with a reflection level left to carry the moved normal on
    live = 0
    for case in D.CASES:
        h, cand, stable = fx.candidates(case)
        for k, c in enumerate(cand):
            live += int((c & ~stable & ((h[:, 6].astype(int) >> k) & 1 == 0) & (h[:, 1] < D.MAX_LVL)).sum())
    assert live >= 20, live


@pytest.mark.parametrize("pf", [1, 3])
@pytest.mark.parametrize("case", list(D.CASES))
def test_frames_and_samples(fx, dev, case, pf):
    wf32, wu8, wcounts = fx.want(case, pf)
    P = _rp(case, pf)
    recs = {}
    for knob in (2, 1, 0):
        dev.tune("dark_lights", knob)
        u8, f32, c = dev.render(P, want_f32=True)
        assert _ints(c) == wcounts, (knob, _ints(c), wcounts)
        assert np.array_equal(u8, wu8), (knob, int((u8 != wu8).sum()), np.argwhere(u8 != wu8)[:4].tolist())
        _same_bits(f32, wf32, f"floats, dark_lights {knob}")
        recs[knob], c = dev.trace_frame_samples(P, with_rays=True)
        assert _ints(c) == wcounts
    dev.tune("dark_lights", 1)
    _same_bits(recs[2], recs[0], "samples, dark_lights 2 against 0")
    _same_bits(recs[1], recs[0], "samples, dark_lights 1 against 0")
    r = recs[2].reshape(-1, 9)[:: 1 if pf == 1 else 7]
    op = _op(case, pf)
    with O.spec_pow("twin"):
        want = np.array([fx.orc.trace(op, s[0:3], s[3:6])[0] for s in r], F32)
    _same_bits(r[:, 6:9], want, "samples against the oracle's trace()")


@pytest.mark.parametrize("case", ["front", "dark_middle", "turned"])
def test_debug_trace_records(fx, dev, case):
    """rt_debug_trace walks every ray (it returns the verdicts): its records are the oracle's on 64 pixels, the
    pixels of dark hits first."""
    h, cand, stable = fx.candidates(case)
    dark = np.zeros(len(h), bool)
    for c in cand:
        dark |= c & stable
    px = list(dict.fromkeys(h[dark, 0].astype(int).tolist()))[:48]
    assert len(px) >= 8
    px += [i for i in range(0, D.W * D.H, 97) if i not in px][: 64 - len(px)]
    _, corners, _, _ = D.params(case)
    o, d = D.pixel_rays(corners, D.W, D.H)
    P, op = _rp(case, 1), _op(case, 1)
    for i in px:
        with O.spec_pow("twin"):
            want, wrgb = fx.orc.debug_trace(op, o[i], d[i])
        got, rgb = dev.debug_trace(P, o[i], d[i])
        assert len(got) == len(want), i
        for a, b in zip(got, want):
            assert (a["triangle"], a["level"], a["shadowed"], a["lit"]) == (b["triangle"], b["level"], b["shadowed"], b["lit"]), i
            for k in ("origin", "dest", "hit"):
                _same_bits(a[k], b[k], (i, k))
        _same_bits(rgb, wrgb, (i, "rgb"))


def test_shadow_work_falls_only_where_a_light_is_dark(fx, gpu_available):
    """(A scene of its own whose launches all have one shape, in screen order and unsplit: the counts of two
    launches are compared for equality, and a wave's walk counts depend on which rays share it.)"""
    with R.Scene.load(fx.path, device=0) as dev:
        for k, v in (("wave_steal", 0), ("chain_split", 0), ("batch_order", 0), ("steal_half", 0), ("steal_quarter", 0)):
            dev.tune(k, v)
        _shadow_work(dev)


def _shadow_work(dev):
    def visits(P, knob):
        dev.tune("dark_lights", knob)
        dev.set_profiling(True, count_work=True)
        dev.reset_stats()
        _, _, c = dev.render(P)
        v = dev.work_stats(_capi.KERNEL_SHADOW)[1]
        dev.set_profiling(False)
        return v, _ints(c)
    try:
        # front: secondary hits only, so the default is enough; behind: primary hits, which need 2
        for case, knob in (("front", 1), ("front", 2), ("behind", 2)):
            P = _rp(case, 1)
            (v1, c1), (v0, c0) = visits(P, knob), visits(P, 0)
            print(case, "knob", knob, "shadow node visits", v1, "against", v0)
            assert c1 == c0 and 0 <= v1 < v0, (case, knob, v1, v0)
        # the default leaves first steps alone: at depth 0 nothing changes even where every hit is dark
        P = _rp("behind", 1, max_lvl=0)
        (v1, c1), (v0, c0) = visits(P, 1), visits(P, 0)
        assert c1 == c0 and v1 == v0 and v0 > 0, (v1, v0)
        # one light at the camera, primary hits only: no light is dark anywhere
        P = R.RenderParams(width=D.W, height=D.H, pf=1, max_lvl=0, lights=[list(D.CAM)])
        (v1, c1), (v0, c0) = visits(P, 2), visits(P, 0)
        assert c1 == c0 and v1 == v0 and v0 > 0, (v1, v0)
    finally:
        dev.set_profiling(False)
        dev.tune("dark_lights", 1)


@pytest.mark.parametrize("shape", ["helpers", "no_helpers", "steal", "quad"])
@pytest.mark.parametrize("case,pf", [(c, 1) for c in D.CASES] + [("behind", 2)])
def test_launch_shapes(fx, gpu_available, case, pf, shape):
    """The split tiers with and without shadow helpers (each helper evaluates the rule for the lights of its own
    role), the stealing kernel (a lane whose light is dark sits the walk out and helps) and the quad walk (the
    quarter tier forced, as tests/test_gpu_parity.py does), launch after launch (the first is unordered, later
    ones ordered and split), with the rule at every step."""
    wf32, wu8, wcounts = fx.want(case, pf)
    P = _rp(case, pf)
    with R.Scene.load(fx.path, device=0) as sc:
        sc.tune("dark_lights", 2)
        sc.tune("wave_steal", 1 if shape == "steal" else 0)
        sc.tune("chain_split", 0)
        if shape == "quad":
            sc.tune("steal_half", 0)
            sc.tune("steal_quarter", 4096)
            sc.tune("quad_walk", 1)
        else:
            sc.tune("steal_half", 512)
            sc.tune("steal_quarter", 8)
            sc.tune("split_eighth", 8)
            sc.tune("shadow_helpers", 0 if shape == "no_helpers" else 1)
        for i in range(4):
            u8, f32, c = sc.render(P, want_f32=True)
            assert _ints(c) == wcounts, i
            assert np.array_equal(u8, wu8), (i, int((u8 != wu8).sum()))
            _same_bits(f32, wf32, (shape, i))


@pytest.mark.parametrize("case,knob", [("front", 1), ("dark_middle", 2), ("turned", 2)])
def test_multi_frame_launch(fx, gpu_available, case, knob):
    """rt_render_frames_device (the multi-frame instantiation of the chain kernel): three frames of the case in
    one launch, each the oracle's bytes, launch after launch."""
    import torch
    _, wu8, wcounts = fx.want(case, 1)
    P = _rp(case, 1)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    with R.Scene.load(fx.path, device=0) as sc:
        sc.tune("dark_lights", knob)
        for it in range(4):
            bufs = [torch.full((D.H * D.W * 3,), 7, dtype=torch.uint8, device=dev) for _ in range(3)]
            counts = sc.render_frames_device([P] * 3, 16, 16, [b.data_ptr() for b in bufs], bufs[0].numel(), st.cuda_stream,
                                             want_counts=True)
            torch.cuda.synchronize(dev)
            assert _ints(counts) == [3 * x for x in wcounts], it
            for b in bufs:
                assert np.array_equal(b.cpu().numpy().reshape(D.H, D.W, 3), wu8), it


@pytest.mark.parametrize("edit", [("Ks 0.500000 0.500000 0.500000", "Ks inf inf inf"), ("Ns 96.078431", "Ns 0.000000")],
                         ids=["Ks_inf", "Ns_0"])
def test_materials_that_switch_the_rule_off(workdir, gpu_available, edit):
    """0 * inf is NaN and pow(0, 0) is 1: the terms of a light behind the hit are not zeros, so the rule must not
    fire on the spheres (the material's flag, set at upload; the back plane's material stays finite). Skipping such a
    light would change the picture: the frames are the oracle's."""
    f = Fixture("F3", workdir, mtl_edit=edit, stem="dark_f3_" + edit[1].split()[0].lower() + "_" + edit[1].split()[1].replace(".", ""))
    with R.Scene.load(f.path, device=0) as sc:
        sc.tune("wave_steal", 0)
        for case in ("behind", "dark_middle"):
            wf32, wu8, wcounts = f.want(case, 1)
            assert not np.array_equal(wu8, Fixture("F3", workdir).want(case, 1)[1])   # the edit shows in the picture
            for knob in (2, 1, 0):
                sc.tune("dark_lights", knob)
                u8, f32, c = sc.render(_rp(case, 1), want_f32=True)
                assert _ints(c) == wcounts
                assert np.array_equal(u8, wu8), (case, knob, int((u8 != wu8).sum()))
                _same_bits(f32, wf32, (case, knob))
