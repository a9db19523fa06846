"""The triangle entries (rt_triangle_overlap_device, rt_triangle_collides_device) without a GPU: exported and declared,
the header still C, RT_E_NODEV on a host-only scene before any other check, and the argument errors that can be reached
without a device (a NULL scene refuses every call; the same cases on a device scene, where each is the only thing
wrong, are in tests/test_gpu_triangle_overlap.py), in the C ABI and in the Python methods."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

ENTRIES = ("rt_triangle_overlap_device", "rt_triangle_collides_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("tri") / "t.obj"
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
    for method in ("triangle_overlap_device", "triangle_collides_device"):
        assert callable(getattr(R.Scene, method))
    assert _capi.TRI_COUNT_ALL == 1 << 4
    assert _capi.TRI_COUNT_ALL not in (_capi.RANGE_TO_DEST, _capi.OCCLUDE_ANY_OPAQUE, _capi.MULTI_COUNT_ALL, _capi.NEAR_COUNT_ALL)
    header = open(_capi.HEADER_PATH).read()
    assert "#define RT_TRI_COUNT_ALL (1u << 4)" in header
    hpp = open(os.path.join(ROOT, "include", "raytracert.hpp")).read()
    assert "rt_triangle_overlap_device(scene_" in hpp and "rt_triangle_collides_device(scene_" in hpp


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "raytracert.h"\n'
                   "int (*const f0)(rt_scene *, const void *, int32_t, int32_t, const void *, const void *, const void *, uint32_t,"
                   " int32_t, void *, void *, void *) = rt_triangle_overlap_device;\n"
                   "int (*const f1)(rt_scene *, const void *, int32_t, int32_t, const void *, const void *, uint32_t,"
                   " void *, void *) = rt_triangle_collides_device;\n"
                   "const unsigned flag = RT_TRI_COUNT_ALL;\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _vp(x):
    return None if x is None else C.c_void_p(x)


def _overlap(scene, n=4, stride=3, tris=0x1000, count=None, after=None, self_index=None, flags=0, k=4, out=0x3000, nfound=0x7000):
    """The list entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    h = scene.handle if scene is not None else None
    return _capi.lib().rt_triangle_overlap_device(h, _vp(tris), stride, n, _vp(count), _vp(after), _vp(self_index), flags, k, _vp(out),
                                                  _vp(nfound), None)


def _collides(scene, n=4, stride=3, tris=0x1000, count=None, self_index=None, flags=0, out=0x3000):
    h = scene.handle if scene is not None else None
    return _capi.lib().rt_triangle_collides_device(h, _vp(tris), stride, n, _vp(count), _vp(self_index), flags, _vp(out), None)


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
    "d_self not 4-byte aligned": dict(self_index=0x6001),
    "a high flag bit": dict(flags=1 << 31),
    "RT_NEAR_COUNT_ALL": dict(flags=_capi.NEAR_COUNT_ALL),
    "RT_MULTI_COUNT_ALL": dict(flags=_capi.MULTI_COUNT_ALL),
}
OVERLAP_CASES = dict(SHARED_CASES, **{
    "k 0": dict(k=0),
    "k 17": dict(k=_capi.MULTI_HIT_MAX + 1),
    "k < 0": dict(k=-3),
    "d_tris_out not 4-byte aligned": dict(out=0x3002),
    "d_nfound_out not 4-byte aligned": dict(nfound=0x7001),
    "d_after not 4-byte aligned": dict(after=0x6002),
    "the count flag without d_nfound_out": dict(flags=_capi.TRI_COUNT_ALL, nfound=None),
    "the count flag with another": dict(flags=_capi.TRI_COUNT_ALL | 1),
    "n * k above INT32_MAX": dict(n=(1 << 27) + 1, k=16),
})
COLLIDES_CASES = dict(SHARED_CASES, **{
    "a flag": dict(flags=1),
    "RT_TRI_COUNT_ALL": dict(flags=_capi.TRI_COUNT_ALL),
})


def test_null_scene_is_an_argument_error():
    assert _overlap(None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()
    assert _collides(None) == _capi.RT_E_ARG
    for what, kw in OVERLAP_CASES.items():
        assert _overlap(None, **kw) == _capi.RT_E_ARG, what
    for what, kw in COLLIDES_CASES.items():
        assert _collides(None, **kw) == _capi.RT_E_ARG, what


def test_host_only_scene_has_no_device(host_scene):
    assert _overlap(host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    assert _collides(host_scene) == _capi.RT_E_NODEV
    # ... and that is checked before every other argument
    for what, kw in OVERLAP_CASES.items():
        assert _overlap(host_scene, **kw) == _capi.RT_E_NODEV, what
    for what, kw in COLLIDES_CASES.items():
        assert _collides(host_scene, **kw) == _capi.RT_E_NODEV, what
    assert _overlap(host_scene, n=0) == _capi.RT_E_NODEV
    assert _collides(host_scene, n=0) == _capi.RT_E_NODEV


def test_python_methods_refuse_bad_arguments_before_any_device(host_scene):
    import torch
    good = torch.zeros((5, 3, 3), dtype=torch.float32)
    bad = {
        "numpy": np.zeros((5, 3, 3), np.float32),
        "cpu tensor": good,
        "float64": torch.zeros((5, 3, 3), dtype=torch.float64),
        "shape (n, 3, 2)": torch.zeros((5, 3, 2), dtype=torch.float32),
        "shape (n, 2, 3)": torch.zeros((5, 2, 3), dtype=torch.float32),
        "shape (n, 4, 3)": torch.zeros((5, 4, 3), dtype=torch.float32),
        "two dimensions": torch.zeros((15, 3), dtype=torch.float32),
        "one dimension": torch.zeros((45,), dtype=torch.float32),
        "non-contiguous": torch.zeros((5, 3, 6), dtype=torch.float32)[:, :, ::2],
    }
    for what, x in bad.items():
        with pytest.raises(ValueError):
            host_scene.triangle_overlap_device(x, 4)
        with pytest.raises(ValueError):
            host_scene.triangle_collides_device(x)
    for k in (0, 17, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="k must be"):
            host_scene.triangle_overlap_device(good, k)
