"""The material gallery shared by tests/test_gallery.py (what the oracle alone says about it) and
tests/test_gpu_gallery.py (the kernels' shading against the oracle, bit for bit).

Scene: one 0.4 x 0.4 tile of two triangles per palette entry in the plane z = 0 (normal +z), on a grid of
pitch 0.5 with six tiles per row, centred on the origin; a backdrop at z = -1 spanning +-4 (normal +z,
material Back) and a canopy at z = 1.5 (normal -z, material Top): 56 triangles, 29 materials with the
default one. One light above the tiles and one below. Coordinates and material values are written with
nine significant digits, so the files hold the float32 values exactly.

Palette: every branch of shade() and refraction() (raytracing.cpp:290-368) has an entry whose colour would
change if the branch were taken wrongly: unequal channels of Ks (a swap shows), Ks different from 1 - Tr (the two
child coefficients), every material flag absent once (the No* blocks, which inherit the values of the block
before them as Mesh::loadMtl does), Ns of 0, 1, fractional, large and negative, Ni below, at and above 1, zero
and negative, Tr at 0, just below 1, above 1 and negative, Ks above 1.

Rays: the list G (K rays from above and K from below per tile, default_rng(21)) and two views of 96 x 80
pixels. Cameras: the default one and one below the scene, for which H.n <= 0 on the tiles seen from above.
"""
from __future__ import annotations

import os

import numpy as np

import oracle as O

F32 = np.float32
PITCH, TILE, INNER, PER_ROW = 0.5, 0.4, 0.36, 6
LIGHTS = [[0.3, 0.2, 1.0], [-0.4, 0.1, -0.6]]
CAMERAS = {"default": (0.0, 0.0, 4.0), "below": (0.2, -0.1, -4.0)}
VIEW_W, VIEW_H, MAX_LVL = 96, 80, 4
VIEW_Z0 = {"above": 1.0, "below": -0.8}
RAY_SEED = 21
K = 32                          # rays per tile and side (tests/test_gallery.py says why not 16)
ACOS_LE2 = float(np.array([0xBED51136], np.uint32).view(F32)[0])   # 0 < acosf(c) <= 2 <=> c >= this, on [-1, 0)

AMBIENT, DIFFUSE, SPECULAR, REFLECTION, SHADOWS, REFRACTION = (1 << i for i in range(6))
ALL = 0x3F
FLAG_SETS = [("all", ALL)] + [(f"no_{n}", ALL & ~b) for n, b in (
    ("ambient", AMBIENT), ("diffuse", DIFFUSE), ("specular", SPECULAR), ("reflection", REFLECTION), ("shadows", SHADOWS),
    ("refraction", REFRACTION))] + [("no_refraction_no_reflection", ALL & ~(REFRACTION | REFLECTION)),
                                    ("ambient_only", AMBIENT), ("none", 0)]

# ---- palette: (name, keys written, in file order Ka Kd Ks Ns Ni d) -----------------------------------
_NS = dict(Ka=(0, 0, 0), Kd=(.3, .3, .3), Ks=(.4, .6, .8), Ni=1, d=1)
_GLASS = dict(Ka=(0, 0, 0), Kd=(.6, .7, .8), Ks=(.5, .4, .3), Ns=96.078431, Ni=1.5, d=0.5)
_BIG = dict(Ka=(.05, .02, .01), Kd=(.1, .1, .1), Ks=(1.5, 1, 2), Ns=20, Ni=1, d=1)


def _without(block, key):
    return {k: v for k, v in block.items() if k != key}


PALETTE = [
    ("Matte", dict(Ka=(.05, .02, .01), Kd=(.7, .3, .2), Ks=(0, 0, 0), Ns=10, Ni=1, d=1)),
    ("Gloss", dict(Ka=(0, 0, 0), Kd=(.2, .5, .8), Ks=(.9, .5, .1), Ns=96.078431, Ni=1, d=1)),
    ("Ns0", dict(_NS, Ns=0)), ("Ns1", dict(_NS, Ns=1)), ("NsHalf", dict(_NS, Ns=0.5)), ("Ns2", dict(_NS, Ns=2)),
    ("Ns1000", dict(_NS, Ns=1000)), ("Ns1e4", dict(_NS, Ns=10000)),
    ("NsNeg", dict(_NS, Ks=(.4, 0, .8), Ns=-1)),           # the zero channel makes 0 * inf
    ("Glass15", dict(_GLASS)),
    ("Water", dict(_GLASS, Ns=50, Ni=1.33, d=0.25)),
    ("Diamond", dict(_GLASS, Ni=2.4, d=0.1)),
    ("Ni1", dict(_GLASS, Ni=1)),
    ("NiLow", dict(_GLASS, Ni=0.75)),
    ("Ni0", dict(_GLASS, Ni=0)),
    ("NiNeg", dict(_GLASS, Ni=-1.5)),
    ("Tr0", dict(_GLASS, Ka=(.1, .1, .1), d=0)),
    ("TrEdge", dict(_GLASS, d=0.99999994)),                 # the largest float below 1
    ("TrOver", dict(_GLASS, d=1.5)),
    ("TrNeg", dict(_GLASS, d=-0.5)),
    ("KsBig", dict(_BIG)),
    ("NoKa", _without(_BIG, "Ka")), ("NoKd", _without(_BIG, "Kd")), ("NoKs", _without(_BIG, "Ks")),
    ("NoNs", _without(_BIG, "Ns")), ("NoD", _without(dict(_BIG, Ni=1.5), "d")),
]
SURROUND = [
    ("Back", dict(Ka=(0, 0, 0), Kd=(.8, .8, .2), Ks=(.2, .3, .4), Ns=30, Ni=1, d=1)),
    ("Top", dict(Ka=(0, 0, 0), Kd=(.2, .8, .8), Ks=(.6, .5, .4), Ns=30, Ni=1, d=1)),
]
NAMES = [n for n, _ in PALETTE]
N_TILES = len(PALETTE)
TRANSPARENT_PATH = ("Glass15", "Water", "Diamond", "Ni1", "NiLow", "Ni0", "NiNeg", "Tr0", "TrEdge", "TrNeg")
OPAQUE_PATH = tuple(n for n in NAMES if n not in TRANSPARENT_PATH)     # TrOver, NoD and every opaque entry
HAS = dict(Kd=1 << 0, Ka=1 << 1, Ks=1 << 2, Ns=1 << 3, Ni=1 << 4, d=1 << 5)      # ORA_HAS_* (oracle/rt_oracle.h)
_FIELD = dict(Kd="Kd", Ka="Ka", Ks="Ks", Ns="Ns", Ni="Ni", d="Tr")


def blocks():
    """The MTL blocks in file order: the surroundings, then the palette (the No* blocks last)."""
    return SURROUND + PALETTE


def expected_materials():
    """What Mesh::loadMtl makes of the file: index 0 the default material, then one per block; a key a block
    does not write keeps the value of the block before it, with its flag clear (mesh.cpp:334-460)."""
    state = dict(Kd=(0, 0, 0), Ka=(0, 0, 0), Ks=(0, 0, 0), Ns=0.0, Ni=0.0, Tr=0.0)
    out = []
    for name, keys in blocks():
        flags = 0
        for k, v in keys.items():
            state[_FIELD[k]] = tuple(float(F32(x)) for x in v) if isinstance(v, tuple) else float(F32(v))
            flags |= HAS[k]
        out.append((name, dict(state, flags=flags)))
    return out


def tile_centre(t: int):
    rows = (N_TILES + PER_ROW - 1) // PER_ROW
    return ((t % PER_ROW) - (PER_ROW - 1) / 2) * PITCH, ((t // PER_ROW) - (rows - 1) / 2) * PITCH


def _quad(x0, y0, x1, y1, z, up: bool):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [a, b, c, d] if up else [a, d, c, b]       # counter-clockwise seen from +z: normal +z


def vertices(scale: float = 1.0) -> np.ndarray:
    """[4 * (N_TILES + 2), 3] float32: the tiles' corners, the backdrop's, the canopy's."""
    v = []
    for t in range(N_TILES):
        cx, cy = tile_centre(t)
        v += _quad(cx - TILE / 2, cy - TILE / 2, cx + TILE / 2, cy + TILE / 2, 0.0, True)
    v += _quad(-4, -4, 4, 4, -1.0, True)
    v += _quad(-4, -4, 4, 4, 1.5, False)
    return (np.asarray(v, np.float64).astype(F32) * F32(scale)).astype(F32)


def _fmt(v):
    return " ".join("%.9g" % F32(x) for x in v) if isinstance(v, tuple) else "%.9g" % F32(v)


def write_scene(directory: str, stem: str = "gallery", scale: float = 1.0, canopy: str = "Top") -> str:
    """The OBJ/MTL pair; returns the OBJ path. scale: every coordinate times it (a power of two is exact);
    canopy: the material name of the canopy's two triangles."""
    with open(os.path.join(directory, stem + ".mtl"), "w", newline="\n") as f:
        for name, keys in blocks():
            f.write(f"newmtl {name}\n")
            for k, v in keys.items():
                f.write(f"{k} {_fmt(v)}\n")
            f.write("illum 2\n\n")
    v = vertices(scale)
    path = os.path.join(directory, stem + ".obj")
    with open(path, "w", newline="\n") as f:
        f.write(f"mtllib {stem}.mtl\n")
        for p in v:
            f.write("v %.9g %.9g %.9g\n" % (p[0], p[1], p[2]))
        for q, name in enumerate(NAMES + ["Back", canopy]):
            f.write("usemtl %s\nf %d %d %d\nf %d %d %d\n" % (name, 4 * q + 1, 4 * q + 2, 4 * q + 3, 4 * q + 1, 4 * q + 3, 4 * q + 4))
    return path


def tile_of_triangle(tri: int) -> int:
    """The palette index of a tile's triangle, N_TILES for the backdrop, N_TILES + 1 for the canopy, -1 for a miss."""
    return tri // 2 if tri >= 0 else -1


def rays(k: int = K, seed: int = RAY_SEED, scale: float = 1.0):
    """The list G: per tile, k rays from above then k from below, (origins, dests, tile, above) in float32. The
    destination is a uniform point of the tile's inner 0.36 x 0.36, the origin 0.8 away from it in a uniform
    direction of that side's hemisphere."""
    rng = np.random.default_rng(seed)
    o, d, tile, above = [], [], [], []
    for t in range(N_TILES):
        cx, cy = tile_centre(t)
        for side in (1.0, -1.0):
            p = np.zeros((k, 3))
            p[:, 0] = cx + rng.uniform(-INNER / 2, INNER / 2, k)
            p[:, 1] = cy + rng.uniform(-INNER / 2, INNER / 2, k)
            u = rng.standard_normal((k, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            u[:, 2] = np.abs(u[:, 2]) * side
            p = p.astype(F32)
            o.append((p + F32(0.8) * u.astype(F32)).astype(F32))
            d.append(p)
            tile += [t] * k
            above += [side > 0] * k
    o, d = np.concatenate(o), np.concatenate(d)
    return (o * F32(scale)).astype(F32), (d * F32(scale)).astype(F32), np.asarray(tile), np.asarray(above)


def view_corners(name: str) -> np.ndarray:
    """Origin corners (+-0.6, +-0.5, z0), dest corners (+-1.6, +-1.35, 0), the signs those of default_corners."""
    sg = np.sign(O.default_corners(VIEW_W, VIEW_H)[:, :2])
    cs = np.zeros((8, 3), F32)
    cs[0::2, :2] = sg[0::2] * np.array([0.6, 0.5], F32)
    cs[0::2, 2] = VIEW_Z0[name]
    cs[1::2, :2] = sg[1::2] * np.array([1.6, 1.35], F32)
    return cs


def ring_lights(n: int = 16):
    """The two lights and n more on a circle of radius 1 at z = 0.8: more than RT_MAX_LIGHTS."""
    a = 2 * np.pi * np.arange(n) / n
    return LIGHTS + [[float(F32(np.cos(t))), float(F32(np.sin(t))), 0.8] for t in a]


def params(flags: int = ALL, camera: str = "default", max_lvl: int = MAX_LVL, lights=None, view: str | None = None, pf: int = 1):
    """Oracle parameters for the list (any frame size) or a view."""
    return O.make_params(VIEW_W, VIEW_H, pf=pf, max_lvl=max_lvl, lights=LIGHTS if lights is None else lights, flags=flags,
                         camera_pos=CAMERAS[camera], corners=view_corners(view or "above"))


def trace_list(orc, p, o, d):
    """(rgb[n, 3], counts[3]) of the oracle over a ray list."""
    rgb = np.zeros((len(o), 3), F32)
    counts = np.zeros(3, np.uint64)
    for i in range(len(o)):
        c, n = orc.trace(p, o[i], d[i])
        rgb[i] = c
        counts += n
    return rgb, counts


def same_bits(a, b) -> bool:
    """Bytes equal, any NaN equal to any NaN (0 * inf is a different NaN on x86 and on the GPU)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def first_difference(a, b):
    """For an assertion message: how many entries differ (NaN equal to NaN) and the first few of them."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    where = np.argwhere(bad)[:4]
    return int(bad.sum()), [(tuple(int(x) for x in w), float(a[tuple(w)]), float(b[tuple(w)])) for w in where]


# ---- coverage: what shade() did at every bounce --------------------------------------------------------
def _check_of(bounce, normal) -> F32:
    """refraction()'s `check` (raytracing.cpp:293-294) in the reference's float operations."""
    ray = (bounce["dest"] - bounce["origin"]).astype(F32)
    length = np.sqrt(F32(F32(ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]), dtype=F32)
    if length != 0:
        ray = (ray * (F32(1) / length)).astype(F32)
    return F32(F32(ray[0] * normal[0] + ray[1] * normal[1]) + ray[2] * normal[2])


def classify(bounces, scene, flags: int, max_lvl: int):
    """One (class, tile) per trace() call of a chain (oracle.debug_trace's bounces, scene = the oracle's
    export): 'miss'; 'mirror', 'enter' or 'exit' with '+child' or '+zero' for the three branches of refraction()
    (zero: it returned black without tracing on); 'reflect'; 'leaf' (no child asked for)."""
    out = []
    for i, b in enumerate(bounces):
        tri = b["triangle"]
        if tri < 0:
            out.append(("miss", -1))
            continue
        m = scene["materials"][int(scene["tri_mat"][tri])]
        deeper = b["level"] < max_lvl
        if (flags & REFRACTION) and F32(m["Tr"]) < 1 and deeper:
            c = _check_of(b, scene["normals"][tri])
            kind = ("mirror" if c >= F32(ACOS_LE2) else "enter") if c < 0 else "exit"
            child = i + 1 < len(bounces)
            assert child or kind != "mirror"
            out.append((kind + ("+child" if child else "+zero"), tile_of_triangle(tri)))
        elif (flags & REFLECTION) and deeper:
            assert i + 1 < len(bounces)
            out.append(("reflect", tile_of_triangle(tri)))
        else:
            assert i + 1 == len(bounces)
            out.append(("leaf", tile_of_triangle(tri)))
    return out


def coverage(orc, p, o, d, flags: int = ALL, max_lvl: int = MAX_LVL):
    """({(class, tile name): bounces}, chain lengths[n]) of the oracle's debug traces of a ray list."""
    scene = orc.export()
    names = NAMES + ["Back", "Top"]
    counts, lengths = {}, np.zeros(len(o), np.int64)
    for i in range(len(o)):
        bounces, _ = orc.debug_trace(p, o[i], d[i])
        lengths[i] = len(bounces)
        for cls, tile in classify(bounces, scene, flags, max_lvl):
            key = (cls, names[tile] if tile >= 0 else None)
            counts[key] = counts.get(key, 0) + 1
    return counts, lengths
