"""The triangle-distance entries (rt_triangle_distance_device, rt_triangle_within_device) without a GPU: exported and
declared, the header still C, the C++ wrappers, RT_E_NODEV on a host-only scene before any other check, the argument
errors that can be reached without a device (a NULL scene refuses every call; the same cases on a device scene, where
each is the only thing wrong, are in tests/test_gpu_triangle_distance.py), in the C ABI and in the Python methods, and
the entries' rules in raytracert_amd/csrc/query_args.h driven on the host by a stand-alone program
(tests/cxx/triangle_distance_args_check.cpp), also built with the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

ENTRIES = ("rt_triangle_distance_device", "rt_triangle_within_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = 10 + 8        # per entry, in the header's order: the five of the arrays, then the entry's own


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("tridist") / "t.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with R.Scene.load(str(p), device=R.RT_HOST_ONLY) as s:
        yield s


def test_entries_are_exported_and_declared():
    lib = _capi.lib()
    declared = _capi.header_symbols(_capi.HEADER_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in _capi._SIGNATURES, name
    assert len(_capi._SIGNATURES["rt_triangle_distance_device"][0]) == 12
    assert len(_capi._SIGNATURES["rt_triangle_within_device"][0]) == 10
    for method in ("triangle_distance", "triangle_within"):
        assert callable(getattr(R.Scene, method))
        assert "_device suffix" in getattr(R.Scene, method).__doc__
    hpp = open(os.path.join(ROOT, "include", "raytracert.hpp")).read()
    assert "rt_triangle_distance_device(scene_" in hpp and "rt_triangle_within_device(scene_" in hpp
    assert "void triangle_distance_device(" in hpp and "void triangle_within_device(" in hpp


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "raytracert.h"\n'
                   "int (*const f0)(rt_scene *, const void *, int32_t, int32_t, const void *, const void *, const void *, uint32_t,"
                   " void *, void *, void *, void *) = rt_triangle_distance_device;\n"
                   "int (*const f1)(rt_scene *, const void *, int32_t, int32_t, const void *, const void *, const void *, uint32_t,"
                   " void *, void *) = rt_triangle_within_device;\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _vp(x):
    return None if x is None else C.c_void_p(x)


def _distance(scene, n=4, stride=3, tris=0x1000, count=None, rmax=None, self_index=None, flags=0, out=0x3000, qpoint=None, point=None):
    """The record entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    h = scene.handle if scene is not None else None
    return _capi.lib().rt_triangle_distance_device(h, _vp(tris), stride, n, _vp(count), _vp(rmax), _vp(self_index), flags, _vp(out),
                                                   _vp(qpoint), _vp(point), None)


def _within(scene, n=4, stride=3, tris=0x1000, count=None, rmax=None, self_index=None, flags=0, out=0x3000):
    h = scene.handle if scene is not None else None
    return _capi.lib().rt_triangle_within_device(h, _vp(tris), stride, n, _vp(count), _vp(rmax), _vp(self_index), flags, _vp(out), None)


# the RT_E_ARG cases (include/raytracert.h), as keyword changes of a call that is otherwise in order
SHARED_CASES = {
    "n < 0": dict(n=-1),
    "stride": dict(stride=5),
    "stride 0": dict(stride=0),
    "stride 9": dict(stride=9),
    "null triangles": dict(tris=None),
    "packed triangles not 4-byte aligned": dict(tris=0x1002),
    "padded triangles not 16-byte aligned": dict(stride=4, tris=0x1004),
    "null output": dict(out=None),
    "d_count not 4-byte aligned": dict(count=0x5002),
    "d_rmax not 4-byte aligned": dict(rmax=0x5001),
    "d_self not 4-byte aligned": dict(self_index=0x6001),
    "a flag": dict(flags=1),
    "a high flag bit": dict(flags=1 << 31),
    "RT_TRI_COUNT_ALL": dict(flags=_capi.TRI_COUNT_ALL),
    "RT_NEAR_COUNT_ALL": dict(flags=_capi.NEAR_COUNT_ALL),
}
DISTANCE_CASES = dict(SHARED_CASES, **{
    "d_hit_out not 16-byte aligned": dict(out=0x3008),
    "d_hit_out 4-byte aligned only": dict(out=0x3004),
    "d_qpoint_out not 4-byte aligned": dict(qpoint=0x7002),
    "d_point_out not 4-byte aligned": dict(point=0x8001),
})


def test_null_scene_is_an_argument_error():
    assert _distance(None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()
    assert _within(None) == _capi.RT_E_ARG
    for what, kw in DISTANCE_CASES.items():
        assert _distance(None, **kw) == _capi.RT_E_ARG, what
    for what, kw in SHARED_CASES.items():
        assert _within(None, **kw) == _capi.RT_E_ARG, what


def test_host_only_scene_has_no_device(host_scene):
    assert _distance(host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    assert _within(host_scene) == _capi.RT_E_NODEV
    # ... and that is checked before every other argument
    for what, kw in DISTANCE_CASES.items():
        assert _distance(host_scene, **kw) == _capi.RT_E_NODEV, what
    for what, kw in SHARED_CASES.items():
        assert _within(host_scene, **kw) == _capi.RT_E_NODEV, what
    assert _distance(host_scene, n=0) == _capi.RT_E_NODEV
    assert _within(host_scene, n=0) == _capi.RT_E_NODEV


def test_python_methods_refuse_bad_arguments_before_any_device(host_scene):
    import torch
    good = torch.zeros((5, 3, 3), dtype=torch.float32)
    bad = {
        "numpy": np.zeros((5, 3, 3), np.float32),
        "cpu tensor": good,
        "float64": torch.zeros((5, 3, 3), dtype=torch.float64),
        "shape (n, 3, 2)": torch.zeros((5, 3, 2), dtype=torch.float32),
        "shape (n, 2, 3)": torch.zeros((5, 2, 3), dtype=torch.float32),
        "two dimensions": torch.zeros((15, 3), dtype=torch.float32),
        "non-contiguous": torch.zeros((5, 3, 6), dtype=torch.float32)[:, :, ::2],
    }
    for what, x in bad.items():
        with pytest.raises(ValueError):
            host_scene.triangle_distance(x)
        with pytest.raises(ValueError):
            host_scene.triangle_within(x)


def _build(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I" + os.path.join(ROOT, "raytracert_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "triangle_distance_args_check.cpp"), "-o", out], check=True)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-4000:] + r.stderr[-4000:]
    return int(r.stdout.split()[1])


def test_argument_rules_on_the_host(tmp_path):
    exe = str(tmp_path / "triangle_distance_args_check")
    _build(exe)
    assert _run(exe) == RULES   # (no entry and no rule skipped)


def test_argument_rules_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "triangle_distance_args_check_san")
    try:
        _build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build the stand-alone check with -fsanitize=address,undefined")
    assert _run(exe) == RULES
