"""What the oracle alone says about the material gallery (tests/_gallery.py), so that no test of
tests/test_gpu_gallery.py passes empty: the file means what the palette table says, every ray of the list G
meets its own tile first, and the list reaches every branch of shade() and refraction() often enough.

K = 32 rays per tile and side (1,664 rays, default_rng(21)). With K = 16 every bar below is met too, but the
fewest mirror bounces of a transparent entry are then exactly the 4 asked for (Ni1); 32 leaves room.

Counts the oracle gives (twin specular power, RT_ALL_FEATURES, max_lvl 4, default camera unless said):
  bounces by class   reflect 2735, leaf 274, miss 1155, mirror 124, enter 245 (55 without a child),
                     exit 357 (180 without a child)
  per entry (mirror, enter, exit)
                     Glass15 12 24 38, Water 14 18 36, Diamond 15 17 35, Ni1 11 23 35, NiLow 16 19 39, Ni0 18 48 34,
                     NiNeg 11 23 33, Tr0 10 24 35, TrEdge 7 25 36, TrNeg 10 24 36
  zero-child         exits: Glass15 28, Water 23, Diamond 34, NiNeg 20, Tr0 25, TrEdge 25, TrNeg 25 (total
                     internal reflection); entries: Ni0 48 (1 / Ni = inf), NiLow 7
  chain lengths 1-5  198, 415, 499, 395, 157
  camera (0.2, -0.1, -4), shadows off
                     rays with an infinite component 73 and with a NaN component 73 (NsNeg: powf(0, -1) = inf
                     times Ks 0.4 0 0.8), above 1: 577, negative: 36
  shadows on         exactly black rays 522 (isShadow's ray is a half-line: past the light it meets the canopy
                     or the backdrop, so a point is lit only through a transparent tile)
  rays whose colour differs from RT_ALL_FEATURES'
                     no_ambient 482, no_diffuse 208, no_specular 848, no_reflection 613, no_shadows 1629,
                     no_refraction 446, no_refraction_no_reflection 694, ambient_only 854, none 1142
  twin against glibc values that differ at all: G default camera 3 of 4992, G camera below (shadows off) 0 of 4992,
                     view above 1 of 23040, view below 1 of 23040 (shadows off); the largest difference is
                     6e-8 of max(1, |value|)
"""
import numpy as np
import pytest

import oracle as O

import _gallery as G

F32_TOL = 2e-6                 # the suite's float RGB tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def gal(workdir):
    path = G.write_scene(workdir)
    orc = O.OracleScene(path)
    o, d, tile, above = G.rays()
    return dict(path=path, orc=orc, o=o, d=d, tile=tile, above=above)


@pytest.fixture(scope="module")
def cov(gal):
    with O.spec_pow("twin"):
        counts, lengths = G.coverage(gal["orc"], G.params(), gal["o"], gal["d"])
    print("coverage", sorted(counts.items(), key=str), "lengths", np.bincount(lengths))
    return counts, lengths


def _n(counts, cls, name):
    return sum(v for (c, n), v in counts.items() if n == name and c.split("+")[0] == cls)


def test_the_file_means_what_the_table_says(gal):
    orc = gal["orc"]
    assert orc.counts() == (4 * (G.N_TILES + 2), 56, 29)
    ex = orc.export()
    want = G.expected_materials()
    assert len(ex["materials"]) == 1 + len(want)
    for (name, w), got in zip(want, ex["materials"][1:]):
        for k in ("Kd", "Ka", "Ks"):
            assert tuple(np.float32(x) for x in got[k]) == tuple(np.float32(x) for x in w[k]), (name, k)
        for k in ("Ns", "Ni", "Tr"):
            assert np.float32(got[k]) == np.float32(w[k]), (name, k, got[k], w[k])
        assert got["flags"] & 0x3F == w["flags"], (name, hex(got["flags"]))
    by_name = dict(want)
    assert by_name["NoD"]["Tr"] == 1.0 and not by_name["NoD"]["flags"] & G.HAS["d"]          # inherits d 1
    assert by_name["NoKs"]["Ks"] == (1.5, 1.0, 2.0) and by_name["TrEdge"]["Tr"] < 1 and by_name["Ni0"]["Ni"] == 0
    # tiles in palette order, then the backdrop and the canopy; normals +z, +z, -z
    names = [n for n, _ in want]
    assert [names[m - 1] for m in ex["tri_mat"][0::2]] == G.NAMES + ["Back", "Top"]
    assert np.array_equal(ex["tri_mat"][0::2], ex["tri_mat"][1::2])
    nz = ex["normals"]
    # (z * (1 / |z|) of normalize() may be one ulp below 1)
    assert (nz[:, :2] == 0).all() and (nz[:-2, 2] >= np.float32(1 - 2 ** -24)).all() and (nz[-2:, 2] <= np.float32(2 ** -24 - 1)).all()


def test_every_ray_meets_its_own_tile_first(gal):
    assert len(gal["o"]) == 2 * G.K * G.N_TILES and gal["o"].dtype == np.float32
    for i in range(len(gal["o"])):
        idx, _ = gal["orc"].intersect_mesh(gal["o"][i], gal["d"][i])
        assert G.tile_of_triangle(idx) == gal["tile"][i], i
    assert ((gal["o"][:, 2] > 0) == gal["above"]).all()


def test_every_branch_of_refraction_is_reached(cov):
    counts, _ = cov
    for name in G.TRANSPARENT_PATH:
        got = [_n(counts, c, name) for c in ("mirror", "enter", "exit")]
        assert min(got) >= 4, (name, got)
    zero = {k: v for k, v in counts.items() if k[0].endswith("+zero")}
    assert sum(zero.values()) >= 10
    assert zero.get(("exit+zero", "Glass15"), 0) >= 1 and zero.get(("exit+zero", "Diamond"), 0) >= 1
    assert zero.get(("enter+zero", "Ni0"), 0) >= 1 and zero.get(("enter+zero", "NiLow"), 0) >= 1
    for name in G.OPAQUE_PATH + ("Back", "Top"):
        assert {c for (c, n) in counts if n == name} <= {"reflect", "leaf"}, name
        assert counts.get(("reflect", name), 0) >= 1, name


def test_chains_of_every_length(cov):
    _, lengths = cov
    assert set(range(1, 6)) <= set(lengths.tolist()) and lengths.max() == 5


def test_non_finite_large_and_negative_colours(gal):
    with O.spec_pow("twin"):
        rgb, _ = G.trace_list(gal["orc"], G.params(G.ALL & ~G.SHADOWS, "below"), gal["o"], gal["d"])
        dark, _ = G.trace_list(gal["orc"], G.params(), gal["o"], gal["d"])
    got = dict(inf=int(np.isinf(rgb).any(axis=1).sum()), nan=int(np.isnan(rgb).any(axis=1).sum()),
               above1=int((rgb > 1).any(axis=1).sum()), negative=int((rgb < 0).any(axis=1).sum()),
               black=int((dark.view(np.uint32) == 0).all(axis=1).sum()))
    print(got)
    assert got["inf"] >= 20 and got["nan"] >= 5 and got["above1"] >= 100 and got["negative"] >= 10
    assert got["black"] >= 100


def test_every_flag_set_changes_the_list(gal):
    with O.spec_pow("twin"):
        ref, _ = G.trace_list(gal["orc"], G.params(), gal["o"], gal["d"])
        got = {}
        for name, flags in G.FLAG_SETS[1:]:
            rgb, _ = G.trace_list(gal["orc"], G.params(flags), gal["o"], gal["d"])
            differ = (rgb.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(rgb) & np.isnan(ref))
            got[name] = int(differ.any(axis=1).sum())
    print(got)
    assert len(G.FLAG_SETS) == 10 and G.FLAG_SETS[0] == ("all", O.ALL_FEATURES)
    assert min(got.values()) >= 50, got


def _twin_against_glibc(a, b, what):
    fin = np.isfinite(a) & np.isfinite(b)
    assert G.same_bits(a[~fin], b[~fin]), what
    rel = np.abs(a[fin] - b[fin]) / np.maximum(1, np.abs(b[fin]))
    print(what, "differ", int((a.view(np.uint32) != b.view(np.uint32))[fin].sum()), "of", a.size, "largest", float(rel.max()))
    assert rel.max() <= F32_TOL, (what, float(rel.max()))


def test_twin_oracle_is_the_glibc_oracle_within_the_suites_tolerance(gal):
    orc = gal["orc"]
    for cam in G.CAMERAS:
        p = G.params(G.ALL & ~G.SHADOWS if cam == "below" else G.ALL, cam)
        glibc, gc = G.trace_list(orc, p, gal["o"], gal["d"])
        with O.spec_pow("twin"):
            twin, tc = G.trace_list(orc, p, gal["o"], gal["d"])
        assert np.array_equal(gc, tc)
        _twin_against_glibc(twin, glibc, "G, camera " + cam)
    for view in G.VIEW_Z0:
        p = G.params(G.ALL & ~G.SHADOWS, "default", view=view)
        gf, gu, gc = orc.render(p)
        with O.spec_pow("twin"):
            tf, tu, tc = orc.render(p)
        assert np.array_equal(gc, tc) and int(np.abs(gu.astype(np.int16) - tu.astype(np.int16)).max()) <= 1
        _twin_against_glibc(tf, gf, "view " + view)
        assert (gf > 0).any(axis=2).mean() > 0.5 and len(np.unique(gu.reshape(-1, 3), axis=0)) > 200


def test_the_switch_restores_glibc_and_rejects_other_names(gal):
    p = G.params(G.ALL & ~G.SHADOWS)
    before, _ = G.trace_list(gal["orc"], p, gal["o"][:64], gal["d"][:64])
    with pytest.raises(ValueError):
        O.set_spec_pow("fast")
    with pytest.raises(RuntimeError):
        with O.spec_pow("twin"):
            raise RuntimeError("inside")
    after, _ = G.trace_list(gal["orc"], p, gal["o"][:64], gal["d"][:64])
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert O.lib().ora_set_spec_pow(2) == -1
