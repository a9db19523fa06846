"""The two numerics functions of the device's shade() on their own (rt_diag_math), against their host
statements, bit for bit, over inputs no frame produces.

spec_powf (raytracert_amd/csrc/spec_pow.h as hipcc builds it for the device) against the same header as g++
builds it for the host (oracle/spec_pow_twin.cpp, -O2 -ffp-contract=off): about a million pairs. The header
claims that tests/cxx/spec_pow_check.cpp "checks the same code on the CPU"; this is the test that the device
build gives the host build's bits, so that what tests/test_spec_pow.py says of the one holds for the other,
and so that tests/test_gpu_gallery.py can compare colours with the twin oracle with no tolerance.

glibc_powf2 (the kernels' powf(x, 2) of refraction(): x * x moved one ulp where glibc differs, by a binary
search of the scene's device copy of the tie table) against this platform's libm powf(x, 2): every key of the
built table with both signs, both neighbours of every key, random floats, the edges. For |x| >= 2, infinities
and NaN the function is documented to return x * x, and that is what is asserted: the table ends at 2, since
the argument is a dot product of two unit vectors; there glibc may differ by an ulp, and no ray reaches it.
"""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest

import oracle as O
import raytracert_amd as R
from raytracert_amd import _capi, scenes

import _gallery as G

pytestmark = pytest.mark.gpu

F32 = np.float32
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracert_amd", "build", "powf2_ties.inc")
CHECK_YS = [1, 2, 3, 5, 7.7, 10, 20, 32, 50, 64, 96, 100, 128, 200, 256, 500, 1000, 1e4, 0.5, 0.1, -1, -3.5]   # spec_pow_check.cpp
PALETTE_NS = sorted({float(F32(keys["Ns"])) for _, keys in G.blocks() if "Ns" in keys})
SPECIAL_YS = [0.0, -0.0, 0.5, 1, 2, 149, 150, 1e4, 1e30, -1, -3.5, np.inf, -np.inf, np.nan]


@pytest.fixture(scope="module")
def scene(workdir, gpu_available):
    with R.Scene.load(scenes.write_sphere_grid(scenes.F4, workdir, "diag_math"), device=0) as sc:
        yield sc


def _bits_equal(got, want):
    """Positions where the bits differ, any NaN equal to any NaN."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))


def spec_pow_pairs():
    rng = np.random.default_rng(3)
    xs, ys = [], []
    # the distribution of tests/cxx/spec_pow_check.cpp: 30,000 bases per exponent of its list
    per_y = 30000
    for y in CHECK_YS:
        x = rng.uniform(0.0, 1.0000002, per_y).astype(F32)
        small = np.arange(per_y) % 7 == 0
        x[small] = np.ldexp(rng.uniform(0.0, 1.0000002, int(small.sum())), -rng.integers(0, 140, int(small.sum()))).astype(F32)
        xs.append(x)
        ys.append(np.full(per_y, y, F32))
    # the special bases against every Ns of the palette and the special exponents
    one = F32(1)
    sx = np.array([0.0, -0.0, 1.0, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), 0.999999]
                  + [2.0 ** -k for k in range(150)] + [float(np.nextafter(F32(0), one))], F32)
    sy = np.array(PALETTE_NS + SPECIAL_YS, F32)
    gx, gy = np.meshgrid(sx, sy, indexing="ij")
    xs.append(gx.ravel())
    ys.append(gy.ravel())
    # ... and random bases of [0, 1] against them
    rx = rng.uniform(0, 1, 4000).astype(F32)
    gx, gy = np.meshgrid(rx, sy, indexing="ij")
    xs.append(gx.ravel())
    ys.append(gy.ravel())
    # subnormal results (0.5^130 .. 0.5^149 and their surroundings), underflow to 0, overflow to inf
    xs.append(np.full(20, 0.5, F32))
    ys.append(np.arange(130, 150).astype(F32))
    n = 60000
    xs.append(rng.uniform(0.3, 0.8, n).astype(F32))
    ys.append(rng.uniform(60, 260, n).astype(F32))
    xs.append(np.ldexp(rng.uniform(0.5, 1, n), -rng.integers(1, 149, n)).astype(F32))
    ys.append(rng.uniform(0.8, 3.0, n).astype(F32))
    xs.append(np.ldexp(rng.uniform(0.5, 1, n // 4), -rng.integers(20, 149, n // 4)).astype(F32))
    ys.append(-rng.uniform(0.5, 8.0, n // 4).astype(F32))
    return np.concatenate(xs), np.concatenate(ys)


def test_device_spec_pow_is_the_host_twin(scene):
    x, y = spec_pow_pairs()
    assert 900_000 <= len(x) <= 1_200_000
    want = O.spec_pow_twin(x, y)
    # the batch entry is the single-call entry the oracle's switch uses
    for i in np.random.default_rng(4).integers(0, len(x), 2000):
        one = F32(O.lib().ora_spec_pow_twin(float(x[i]), float(y[i])))
        assert _bits_equal([one], [want[i]]).size == 0
    tiny = np.finfo(F32).tiny
    sub = (want != 0) & (np.abs(want) < tiny)
    print("pairs", len(x), "subnormal", int(sub.sum()), "zero", int((want == 0).sum()), "inf", int(np.isinf(want).sum()),
          "nan", int(np.isnan(want).sum()))
    assert sub.sum() >= 1000 and (want == 0).sum() >= 1000 and np.isinf(want).sum() >= 100 and np.isnan(want).sum() >= 100
    got = scene.diag_math("spec_pow", x, y)
    bad = _bits_equal(got, want)
    assert bad.size == 0, (bad.size, [(float(x[i]), float(y[i]), hex(got.view(np.uint32)[i]), hex(want.view(np.uint32)[i]))
                                      for i in bad[:8]])


def _table_keys():
    txt = open(INC).read()
    body = txt[txt.index("{") + 1: txt.index("}")]
    t = np.array([int(v, 16) for v in re.findall(r"0x[0-9a-f]+", body)], np.uint64).astype(np.uint32)
    return t & 0x7FFFFFFF


def test_device_powf2_is_this_platforms_powf(scene):
    keys = _table_keys()
    assert 300000 < len(keys) < 500000 and keys.max() < 0x40000000
    rng = np.random.default_rng(5)
    mag = np.concatenate([keys, keys - 1, keys + 1]).astype(np.uint32)
    mag = mag[mag < 0x40000000].view(F32)
    two = F32(2)
    edges = np.array([0.0, 1.0, np.nextafter(two, F32(0)), np.nextafter(F32(0), two), 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38,
                      0.5, np.nextafter(F32(1), two), np.nextafter(F32(1), F32(0))], F32)
    x = np.concatenate([mag, -mag, rng.uniform(-2, 2, 200000).astype(F32), edges, -edges])
    assert (np.abs(x) < 2).all() and len(x) > 2_000_000
    want = O.libm_powf(x, np.full(len(x), 2, F32))
    # the batch entry is libm's powf, called as tests/test_numerics.py calls it
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.powf.argtypes, libm.powf.restype = [C.c_float, C.c_float], C.c_float
    for i in rng.integers(0, len(x), 5000):
        assert F32(libm.powf(float(x[i]), 2.0)).view(np.uint32) == want.view(np.uint32)[i]
    plain = x * x
    moved = int((plain.view(np.uint32) != want.view(np.uint32)).sum())
    assert moved >= 2 * len(keys)                        # (every key, both signs: the table is not idle)
    got = scene.diag_math("powf2", x)
    bad = _bits_equal(got, want)
    assert bad.size == 0, (bad.size, [(float(x[i]), hex(got.view(np.uint32)[i]), hex(want.view(np.uint32)[i])) for i in bad[:8]])
    # outside the table: x * x, as documented
    big = np.concatenate([[2.0, -2.0, np.nextafter(two, F32(3)), 3.0, 1e10, 1.8446744e19, 1e30, np.inf, -np.inf, np.nan],
                          rng.uniform(2, 100, 2000), -rng.uniform(2, 100, 2000)]).astype(F32)
    with np.errstate(over="ignore"):
        want_big = big * big
    bad = _bits_equal(scene.diag_math("powf2", big), want_big)
    assert bad.size == 0, [float(big[i]) for i in bad[:8]]


SENTINEL = F32(-123.25)


def _raw(handle, kind, x, y, n, out):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    return _capi.lib().rt_diag_math(handle, kind, p(x), p(y), n, p(out))


@pytest.mark.parametrize("case", ["null scene", "host-only scene", "unknown kind", "negative kind", "negative n", "null x",
                                  "null y for spec_pow", "null out"])
def test_argument_errors_leave_out_untouched(scene, workdir, case):
    x, y = np.linspace(0, 1, 8, dtype=F32), np.full(8, 2, F32)
    out = np.full(8, SENTINEL, F32)
    h, kind, n, args = scene.handle, _capi.DIAG_SPEC_POW, 8, [x, y, out]
    host = None
    if case == "null scene":
        h = None
    elif case == "host-only scene":
        host = R.Scene.load(scenes.write_sphere_grid(scenes.F4, workdir, "diag_math"), device=R.RT_HOST_ONLY)
        h = host.handle
    elif case == "unknown kind":
        kind = 2
    elif case == "negative kind":
        kind = -1
    elif case == "negative n":
        n = -1
    elif case == "null x":
        args[0] = None
    elif case == "null y for spec_pow":
        args[1] = None
    elif case == "null out":
        args[2] = None
    assert _raw(h, kind, args[0], args[1], n, args[2]) == _capi.RT_E_ARG
    assert (out == SENTINEL).all()
    if host is not None:
        host.close()


def test_empty_and_optional_arguments(scene):
    x, out = np.array([0.5, -1.5], F32), np.full(2, SENTINEL, F32)
    assert _raw(scene.handle, _capi.DIAG_POWF2, x, None, 0, out) == _capi.RT_OK and (out == SENTINEL).all()      # n == 0
    assert _raw(scene.handle, _capi.DIAG_SPEC_POW, None, None, 0, None) == _capi.RT_OK
    assert _raw(scene.handle, _capi.DIAG_POWF2, x, None, 2, out) == _capi.RT_OK                                  # y may be NULL
    assert out.tolist() == [0.25, 2.25]
    assert scene.diag_math("spec_pow", [0.5, 0.25], [2, 0.5]).tolist() == [0.25, 0.5]
    with pytest.raises(ValueError):
        scene.diag_math("spec_pow", [0.5, 0.25], [2])
