"""Shared by tests/test_gpu_dark_lights.py: the light sets that force each branch of the dark-light rule
(raytracert_amd/csrc/dark_lights.h), the rule restated in numpy binary32, and the oracle's hits to check each
set's preconditions on the CPU."""
import numpy as np

import oracle as O

F32 = np.float32
MARGIN = F32(1e-3)
W, H, MAX_LVL = 96, 54, 3
CAM = (0.0, 0.0, 4.0)
SPECULAR = 1 << 2   # RT_SPECULAR (include/raytracert.h)


def turned_corners(width, height):
    """The default view turned 90 degrees about the y axis: the rays come from +x."""
    c = O.default_corners(width, height).astype(F32)
    out = c.copy()
    out[:, 0] = c[:, 2]
    out[:, 2] = -c[:, 0]
    return out


BACK = (-1.2, -12.0, -2.0)   # below and behind: its rays to the spheres pass under the back plane's edge
# name -> (lights, turned view, camera position, flags). The camera position (the specular term's eye,
# raytracing.cpp:213) is a global of its own, apart from the view's corner rays: put behind the scene, the
# primary hits face away from it, as the hits seen in C4's mirror face away from the real one.
CASES = {
    # 1: the benchmark's C4 pair, the off-axis light pulled in to the 2 x 2 grid: no primary hit is dark, some secondary are
    "front": ([[0.0, 0.0, 4.0], [0.6, 0.6, 4.0]], False, CAM, O.ALL_FEATURES),
    # 2: one light behind the spheres, the eye beside it: most primary hits are dark for it
    "behind": ([list(BACK)], False, BACK, O.ALL_FEATURES),
    # ... and without the specular term (c = 1: one normalisation per light), the eye in front
    "behind_diffuse": ([list(BACK)], False, CAM, O.ALL_FEATURES & ~SPECULAR),
    # 3: the dark light first, in the middle and last among unshadowed ones
    "dark_first": ([list(BACK), [0.0, 0.0, 4.0], [0.6, 0.6, 4.0]], False, BACK, O.ALL_FEATURES),
    "dark_middle": ([[0.0, 0.0, 4.0], list(BACK), [0.6, 0.6, 4.0]], False, BACK, O.ALL_FEATURES),
    "dark_last": ([[0.0, 0.0, 4.0], [0.6, 0.6, 4.0], list(BACK)], False, BACK, O.ALL_FEATURES),
    # 4: a light at the camera position and one opposite it through a point of the back plane that the view,
    # turned 90 degrees, sees: there V + L nearly cancels, and the hit passes the one-dot test of the second
    # light but not the view compare
    "turned": ([[0.0, 0.0, 4.0], [3.37, 0.0, -5.2]], True, CAM, O.ALL_FEATURES),
}


def normalize(n):
    """Vec3D::normalize on rows of float32 (Vec3D.h:142-151): the kernels' operations in their order."""
    n = np.asarray(n, F32)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    ln = np.sqrt((x * x + y * y) + z * z)
    rez = F32(1) / np.where(ln == 0, F32(1), ln)
    out = n * rez[:, None]
    out[ln == 0] = n[ln == 0]
    return out.astype(F32)


def fixed_point(n, c=2):
    """N^c(n) == n bit for bit, per row."""
    m = np.asarray(n, F32)
    for _ in range(c):
        m = normalize(m)
    return (m.view(np.uint32) == np.asarray(n, F32).view(np.uint32)).all(axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _facing(n, v):
    t, vv = _dot(n, v), _dot(v, v)
    return (t < 0) & (t * t >= (MARGIN * MARGIN) * vv)


def candidates(n0, P, light, cam=CAM, spec=True):
    """Dark candidates (every compare of the rule but the fixed point) of hits (normals n0, points P) for one
    light, every material of these scenes having diffuse and specular terms."""
    n0, P = np.asarray(n0, F32), np.asarray(P, F32)
    L = np.asarray(light, F32)[None, :]
    ln = normalize(L)
    side = _dot(n0, np.broadcast_to(ln, n0.shape)) <= -MARGIN
    if not spec:
        return side
    return side & _facing(n0, np.asarray(cam, F32)[None, :] - P) & _facing(n0, L - P)


def params(case, width=W, height=H):
    """(lights, corners, camera position, flags) of a case."""
    lights, turned, cam, flags = CASES[case]
    return lights, (turned_corners(width, height) if turned else O.default_corners(width, height)), cam, flags


def pixel_rays(corners, width, height):
    """Origin and destination of every pixel's ray at pf 1, in binary32 as the 'r' loop makes them (main.cpp:360-386)."""
    c = np.asarray(corners, F32)
    ys, xs = np.mgrid[0:height, 0:width]
    xscale = (F32(1) - xs.reshape(-1, 1).astype(F32) / F32(width - 1)).astype(F32)
    yscale = (F32(1) - ys.reshape(-1, 1).astype(F32) / F32(height - 1)).astype(F32)
    one = F32(1)

    def mix(k):   # corners 2k' + k: k = 0 origins, 1 destinations
        a00, a01, a10, a11 = c[0 + k], c[2 + k], c[4 + k], c[6 + k]
        return ((a00 * xscale + a10 * (one - xscale)) * yscale + (a01 * xscale + a11 * (one - xscale)) * (one - yscale)).astype(F32)
    return mix(0), mix(1)


def hits(orc, case, width=W, height=H, step=1):
    """The oracle's hits along the chains of every `step`-th pixel ray: (pixel, level, triangle, point, isShadow's
    verdicts as bits) rows."""
    lights, cs, cam, flags = params(case, width, height)
    p = O.make_params(width, height, 1, MAX_LVL, lights=lights, corners=cs, camera_pos=cam, flags=flags)
    o, d = pixel_rays(cs, width, height)
    rows = []
    for i in range(0, width * height, step):
        for b in orc.debug_trace(p, o[i], d[i])[0]:
            if b["triangle"] >= 0:
                rows.append((i, b["level"], b["triangle"], *[float(x) for x in b["hit"]], b["shadowed"]))
    return np.array(rows, np.float64).reshape(-1, 7)
