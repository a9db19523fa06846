"""The closest-point entries (rt_closest_point_device, rt_closest_point) without a GPU: exported and declared,
the header still C, RT_E_NODEV on a host-only scene before any other check, and the argument errors that can be
reached without a device (a NULL scene refuses every call; the same cases on a device scene, where each is the
only thing wrong, are in tests/test_gpu_closest_point.py), in the C ABI and in the Python methods."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

ENTRIES = ("rt_closest_point_device", "rt_closest_point")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("cp") / "t.obj"
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
    for method in ("closest_point_device", "closest_point"):
        assert callable(getattr(R.Scene, method))
    hpp = open(os.path.join(ROOT, "include", "raytracert.hpp")).read()
    assert "rt_closest_point_device(scene_" in hpp


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "raytracert.h"\n'
                   "int (*const f0)(rt_scene *, const void *, int32_t, int32_t, const void *, const void *, uint32_t,"
                   " void *, void *, void *) = rt_closest_point_device;\n"
                   "int (*const f1)(rt_scene *, const float *, int32_t, const float *, rt_hit *, float *) = rt_closest_point;\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _call(scene, n=4, stride=3, pts=0x1000, count=None, rmax=None, flags=0, out=0x3000, out2=None):
    """The device entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    h = scene.handle if scene is not None else None
    vp = lambda x: None if x is None else C.c_void_p(x)
    return _capi.lib().rt_closest_point_device(h, vp(pts), stride, n, vp(count), vp(rmax), flags, vp(out), vp(out2), None)


# the RT_E_ARG cases (include/raytracert.h), as keyword changes of a call that is otherwise in order
ARG_CASES = {
    "n < 0": dict(n=-1),
    "stride": dict(stride=5),
    "stride 0": dict(stride=0),
    "null points": dict(pts=None),
    "packed points not 4-byte aligned": dict(pts=0x1002),
    "padded points not 16-byte aligned": dict(stride=4, pts=0x1004),
    "null output": dict(out=None),
    "d_hit_out not 16-byte aligned": dict(out=0x3008),
    "d_point_out not 4-byte aligned": dict(out2=0x4002),
    "d_count not 4-byte aligned": dict(count=0x5002),
    "d_rmax not 4-byte aligned": dict(rmax=0x6001),
    "a flag": dict(flags=1),
    "a high flag bit": dict(flags=1 << 31),
}


def test_null_scene_is_an_argument_error():
    assert _call(None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()
    for what, kw in ARG_CASES.items():
        assert _call(None, **kw) == _capi.RT_E_ARG, what
    pts = np.zeros((4, 3), np.float32)
    rec = np.zeros((4, 4), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _capi.lib().rt_closest_point(None, vp(pts), 4, None, vp(rec), None) == _capi.RT_E_ARG


def test_host_only_scene_has_no_device(host_scene):
    assert _call(host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    # ... and that is checked before every other argument
    for what, kw in ARG_CASES.items():
        assert _call(host_scene, **kw) == _capi.RT_E_NODEV, what
    assert _call(host_scene, n=0) == _capi.RT_E_NODEV
    with pytest.raises(R.RtError):
        host_scene.closest_point(np.zeros((4, 3), np.float32))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pts, rec = np.zeros((4, 3), np.float32), np.zeros((4, 4), np.int32)
    assert _capi.lib().rt_closest_point(host_scene.handle, vp(pts), 4, None, vp(rec), None) == _capi.RT_E_NODEV
    assert _capi.lib().rt_closest_point(host_scene.handle, None, -1, None, None, None) == _capi.RT_E_NODEV


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
            host_scene.closest_point_device(x)
    with pytest.raises(ValueError, match="closest_point"):   # the message points to the host method
        host_scene.closest_point_device(bad["numpy"])
    with pytest.raises(ValueError, match="rmax"):
        host_scene.closest_point(np.zeros((5, 3), np.float32), rmax=np.zeros(4, np.float32))
