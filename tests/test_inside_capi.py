"""The inside entries (rt_point_inside_device, rt_signed_distance_device) without a GPU: exported and declared, the
header still C, RT_E_NODEV on a host-only scene before any other check, and the argument errors that can be reached
without a device (a NULL scene refuses every call; the same cases on a device scene, where each is the only thing
wrong, are in tests/test_gpu_inside.py), in the C ABI and in the Python methods."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

ENTRIES = ("rt_point_inside_device", "rt_signed_distance_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("inside") / "t.obj"
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
    for method in ("point_inside_device", "signed_distance_device"):
        assert callable(getattr(R.Scene, method))
    axes = (_capi.AXIS_POS_X, _capi.AXIS_NEG_X, _capi.AXIS_POS_Y, _capi.AXIS_NEG_Y, _capi.AXIS_POS_Z, _capi.AXIS_NEG_Z)
    assert axes == (0, 1, 2, 3, 4, 5)
    header = open(_capi.HEADER_PATH).read()
    for name, value in zip(("POS_X", "NEG_X", "POS_Y", "NEG_Y", "POS_Z", "NEG_Z"), axes):
        assert f"#define RT_AXIS_{name} {value}\n" in header
    hpp = open(os.path.join(ROOT, "include", "raytracert.hpp")).read()
    assert "rt_point_inside_device(scene_" in hpp and "rt_signed_distance_device(scene_" in hpp


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "raytracert.h"\n'
                   "int (*const f0)(rt_scene *, const void *, int32_t, int32_t, const void *, int32_t, uint32_t,"
                   " void *, void *, void *) = rt_point_inside_device;\n"
                   "int (*const f1)(rt_scene *, const void *, int32_t, int32_t, const void *, const void *, int32_t, uint32_t,"
                   " void *, void *, void *, void *) = rt_signed_distance_device;\n"
                   "const int axes[6] = {RT_AXIS_POS_X, RT_AXIS_NEG_X, RT_AXIS_POS_Y, RT_AXIS_NEG_Y, RT_AXIS_POS_Z, RT_AXIS_NEG_Z};\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _vp(x):
    return None if x is None else C.c_void_p(x)


def _inside(scene, n=4, stride=3, pts=0x1000, count=None, axis=4, flags=0, out=0x3000, crossings=0x7000):
    """The verdict entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    h = scene.handle if scene is not None else None
    return _capi.lib().rt_point_inside_device(h, _vp(pts), stride, n, _vp(count), axis, flags, _vp(out), _vp(crossings), None)


def _signed(scene, n=4, stride=3, pts=0x1000, count=None, rmax=None, axis=4, flags=0, out=0x3000, out2=None, inside=None):
    h = scene.handle if scene is not None else None
    return _capi.lib().rt_signed_distance_device(h, _vp(pts), stride, n, _vp(count), _vp(rmax), axis, flags, _vp(out), _vp(out2),
                                                 _vp(inside), None)


# the RT_E_ARG cases (include/raytracert.h), as keyword changes of a call that is otherwise in order
SHARED_CASES = {
    "n < 0": dict(n=-1),
    "stride": dict(stride=5),
    "stride 0": dict(stride=0),
    "null points": dict(pts=None),
    "packed points not 4-byte aligned": dict(pts=0x1002),
    "padded points not 16-byte aligned": dict(stride=4, pts=0x1004),
    "null output": dict(out=None),
    "d_count not 4-byte aligned": dict(count=0x5002),
    "a flag": dict(flags=1),
    "a high flag bit": dict(flags=1 << 31),
    "RT_NEAR_COUNT_ALL": dict(flags=_capi.NEAR_COUNT_ALL),
    "axis -1": dict(axis=-1),
    "axis 6": dict(axis=6),
    "axis 1 << 30": dict(axis=1 << 30),
}
INSIDE_CASES = dict(SHARED_CASES, **{
    "d_crossings_out not 4-byte aligned": dict(crossings=0x7002),
})
SIGNED_CASES = dict(SHARED_CASES, **{
    "d_hit_out not 16-byte aligned": dict(out=0x3008),
    "d_point_out not 4-byte aligned": dict(out2=0x4002),
    "d_rmax not 4-byte aligned": dict(rmax=0x6001),
})


def test_null_scene_is_an_argument_error():
    assert _inside(None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()
    assert _signed(None) == _capi.RT_E_ARG
    for what, kw in INSIDE_CASES.items():
        assert _inside(None, **kw) == _capi.RT_E_ARG, what
    for what, kw in SIGNED_CASES.items():
        assert _signed(None, **kw) == _capi.RT_E_ARG, what


def test_host_only_scene_has_no_device(host_scene):
    assert _inside(host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    assert _signed(host_scene) == _capi.RT_E_NODEV
    # ... and that is checked before every other argument
    for what, kw in INSIDE_CASES.items():
        assert _inside(host_scene, **kw) == _capi.RT_E_NODEV, what
    for what, kw in SIGNED_CASES.items():
        assert _signed(host_scene, **kw) == _capi.RT_E_NODEV, what
    assert _inside(host_scene, n=0) == _capi.RT_E_NODEV
    assert _signed(host_scene, n=0) == _capi.RT_E_NODEV


def test_python_methods_refuse_bad_arguments_before_any_device(host_scene):
    import torch
    bad = {
        "numpy": np.zeros((5, 3), np.float32),
        "cpu tensor": torch.zeros((5, 3), dtype=torch.float32),
        "float64": torch.zeros((5, 3), dtype=torch.float64),
        "shape (n, 2)": torch.zeros((5, 2), dtype=torch.float32),
        "one dimension": torch.zeros((15,), dtype=torch.float32),
        "non-contiguous": torch.zeros((5, 6), dtype=torch.float32)[:, ::2],
    }
    for what, x in bad.items():
        with pytest.raises(ValueError):
            host_scene.point_inside_device(x)
        with pytest.raises(ValueError):
            host_scene.signed_distance_device(x)
    for axis in (-1, 6, 2.0, True, None, "z"):
        with pytest.raises(ValueError, match="axis must be"):
            host_scene.point_inside_device(bad["cpu tensor"], axis=axis)
        with pytest.raises(ValueError, match="axis must be"):
            host_scene.signed_distance_device(bad["cpu tensor"], axis=axis)
