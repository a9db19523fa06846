"""What the oracle alone says about the edge-ray classes of tests/_edge_rays.py: the conditions that keep a
case of tests/test_gpu_edge_rays.py from passing empty. (No GPU: the ray queries have no host-only path,
rt_intersect_mesh on a device -1 scene is RT_E_NODEV, so there is no CPU walk to give the same treatment.)

Measured with the seeds of _edge_rays.py (hits / distinct triangles of 256 rays unless noted):
A 192 / 135 (64 misses); B 256 / 167 at each scale, every index the unscaled ray's; C 1e-2 256 / 167, 1e-4
256 / 165, 1e-6 none; D x, y, z 256 each, inside 250, grid 256; E none; F 1e4 256 / 171, 1e7 256 / 80, 1e12
256 / 1 (the reference's rounding), 1e30 none; G 246 / 169; H none (64 rays). Every hit ray of A and B is
accepted by two or more triangles. On the scene scaled by 2^21: A 192, B 247 / 215 / 215, D as unscaled; by
2^10: A 192, B 256 / 256 / 247, D as unscaled.
"""
import numpy as np
import pytest

import oracle as O

import _edge_rays as E


@pytest.fixture(scope="module")
def orc(workdir):
    o = O.OracleScene(E.write_scene(workdir, "shingles_cpu"))
    nv, nt, nm = o.counts()
    assert (nv, nt) == (3 * E.N_TRI, E.N_TRI) and nt % 64 != 0
    # the file holds the float32 coordinates exactly
    assert np.array_equal(o.export()["vertices"].reshape(-1, 3, 3), E.triangles())
    return o


@pytest.fixture(scope="module")
def answers(orc):
    return {name: E.oracle_answers(orc, o, d) for name, (o, d) in E.subclasses().items()}


def _hits(a):
    return int((a["index"] >= 0).sum())


def _distinct(a):
    return len(set(a["index"][a["index"] >= 0]))


def test_class_sizes_and_types():
    sub = E.subclasses()
    assert [n[0] for n in sub] == sorted(n[0] for n in sub) and {n[0] for n in sub} == set("ABCDEFGH")
    for name, (o, d) in sub.items():
        assert len(o) == (64 if name == "H" else 256), name
    # what each construction promises about the direction dest - origin, in float32
    for name in ("D_x", "D_y", "D_z"):
        o, d = sub[name]
        dirs = d - o
        axis = "xyz".index(name[2])
        assert (np.delete(dirs, axis, axis=1) == 0).all() and (dirs[::2, axis] > 0).all() and (dirs[1::2, axis] < 0).all()
        assert (np.abs(o[:, axis]) == 3).all()
    dirs = sub["D_inside"][1] - sub["D_inside"][0]
    assert (dirs[:, 1:] == 0).all() and (dirs[:, 0] > 0).all()
    o, d = sub["D_grid"]
    dirs = d - o
    assert ((dirs == 0).sum(axis=1) == 1).all()
    assert np.signbit(dirs[128:192, 0]).all() and np.signbit(dirs[192:, 1]).all() and not np.signbit(dirs[:64, 0]).any()
    assert np.array_equal(*sub["E"])
    for s in E.B_SCALES:
        o, d = sub["B_" + E._tag(s)]
        dirs = (d - o).astype(np.float32)
        with np.errstate(over="ignore"):
            assert np.isfinite(dirs).all() and np.isinf((dirs * dirs).sum(axis=1, dtype=np.float32)).all()   # dot(dir, dir) overflows
    o, d = sub["H"]
    assert (~np.isfinite(np.concatenate([o, d], axis=1))).any(axis=1).all()
    T = E.triangles()[::11][:64]
    o, d = sub["G"]
    assert np.array_equal(o[:64, :2], T[:, 0, :2]) and np.array_equal(o[192:], T[:, 0]) and np.array_equal(d[64:128], T[:, 1])


def test_generic_rays_hit_miss_and_overlap(answers):
    a = answers["A"]
    assert _hits(a) >= 100 and 256 - _hits(a) >= 30 and _distinct(a) >= 50


@pytest.mark.parametrize("name", ["A"] + ["B_" + E._tag(s) for s in E.B_SCALES])
def test_hit_rays_are_accepted_by_several_triangles(answers, name):
    """The nearest hit is one of several acceptances: a walk that stops at the first leaf's hit is wrong."""
    o, d = E.subclasses()[name]
    hit = answers[name]["index"] >= 0
    acc = E.acceptances(E.triangles(), o, d)
    assert ((acc > 0) == hit).all()
    assert (acc[hit] >= 2).sum() >= 0.9 * hit.sum()


def test_long_rays_hit_what_the_unscaled_rays_hit(orc, answers):
    base = E.oracle_answers(orc, *E.base_rays())
    assert _hits(base) >= 200
    for s in E.B_SCALES:
        a = answers["B_" + E._tag(s)]
        assert _hits(a) >= 200
        assert np.array_equal(a["index"], base["index"])


def test_short_rays(answers):
    assert _hits(answers["C_1e-2"]) >= 200 and _hits(answers["C_1e-4"]) >= 200
    assert _hits(answers["C_1e-6"]) == 0          # |n.dir| < 1e-5 for every triangle


def test_axis_rays(answers):
    for name in ("D_x", "D_y", "D_z", "D_inside", "D_grid"):
        assert _hits(answers[name]) >= 200 and _distinct(answers[name]) >= 50, name


def test_zero_length_rays_hit_nothing(answers):
    assert _hits(answers["E"]) == 0


def test_far_origins(answers):
    assert _hits(answers["F_1e4"]) >= 200 and _distinct(answers["F_1e4"]) >= 50
    assert _hits(answers["F_1e7"]) >= 200 and _distinct(answers["F_1e7"]) >= 50
    assert _hits(answers["F_1e12"]) >= 200        # (one triangle for every ray: the reference's rounding)
    assert _hits(answers["F_1e30"]) == 0          # the distance is not below FLT_MAX


def test_plane_vertex_and_edge_rays(answers):
    a = answers["G"]
    for g in range(4):
        assert (a["index"][64 * g:64 * g + 64] >= 0).sum() >= 32, g


def test_nonfinite_rays_hit_nothing(answers):
    a = answers["H"]
    assert _hits(a) == 0 and (a["point"].view(np.uint32) == 0).all()


def test_prefixes_hold_hits(answers):
    """The prefix counts of the GPU file put hits in the last partial wave."""
    for name in ("A", "B_1e20", "D_x", "F_1e4"):
        hit = answers[name]["index"] >= 0
        for n in E.PREFIXES:
            assert hit[:n].any(), (name, n)


def test_transparent_twin_has_the_same_hits_and_both_verdicts(workdir, answers):
    tr = O.OracleScene(E.write_scene(workdir, "shingles_tr_cpu", transparent=True))
    for name in ("A", "B_1e20", "D_x", "F_1e7"):
        a = E.oracle_answers(tr, *E.subclasses()[name])
        assert np.array_equal(a["index"], answers[name]["index"])
        assert a["transparent_closest"].sum() >= 30 and a["blocked"].sum() >= 30, name
        assert not answers[name]["transparent_closest"].any()


@pytest.mark.parametrize("scale", [E.BIG, E.MID])
def test_scaled_scenes_keep_hits(workdir, scale):
    """Powers of two are exact, but the reference's |n.dir| < 1e-5 test and float range are not scale-free: the
    scaled file's own oracle is the reference of the GPU cases. Where n.dir overflows (2^21: every scale of
    class B; 2^10: 1e30) the reference gets r = a / inf = 0 and I = o, and accepts the triangles whose plane
    projection holds the origin, at distance 0 (measured: 241 / 215 / 215 of 256 at 2^21, 241 at 2^10)."""
    big = O.OracleScene(E.write_scene(workdir, "shingles_scaled_cpu", scale=scale))
    v = big.export()["vertices"]
    assert np.array_equal(v.reshape(-1, 3, 3), E.triangles() * np.float32(scale))
    assert (np.abs(v).sum(axis=1).max() >= 1e6) == (scale == E.BIG)     # scene_m1: which walk is the default
    for letter in "ABD":
        o, d, where = E.class_rays(letter, scale)
        a = E.oracle_answers(big, o, d)
        for name, s in where.items():
            assert (a["index"][s] >= 0).sum() >= (100 if letter == "A" else 200), name
        if letter == "B":
            s = where["B_1e30"]
            assert ((a["point"][s] == o[s]).all(axis=1) & (a["index"][s] >= 0)).sum() >= 200
