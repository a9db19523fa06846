"""rt_multi_hit_range_device without a GPU: exported, declared and bound, its constants, the header still C and the
C++ forwarder compiling, RT_E_NODEV on a host-only scene before any other check, RT_E_ARG for a NULL scene, and the
Python method's checks that come before any device is touched. (The same argument errors on a device scene, where
each is the only thing wrong, are in tests/test_gpu_multi_hit.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

NAME = "rt_multi_hit_range_device"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = ("int (*const f)(rt_scene *, const void *, const void *, int32_t, int32_t, const void *, const void *, const void *,"
         " uint32_t, int32_t, void *, void *, void *) = rt_multi_hit_range_device;\n")


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("mh") / "t.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with R.Scene.load(str(p), device=R.RT_HOST_ONLY) as s:
        yield s


def test_entry_is_exported_declared_and_bound():
    lib = _capi.lib()
    assert hasattr(lib, NAME)
    assert NAME in _capi.header_symbols(_capi.HEADER_PATH)
    args, res = _capi._SIGNATURES[NAME]
    assert len(args) == 13 and res is C.c_int and args[8] is C.c_uint32 and args[9] is C.c_int32
    text = open(_capi.HEADER_PATH).read()
    assert "#define RT_MULTI_HIT_MAX   16" in text and "#define RT_MULTI_COUNT_ALL (1u << 2)" in text
    assert (_capi.MULTI_HIT_MAX, _capi.MULTI_COUNT_ALL) == (16, 4)
    assert _capi.MULTI_COUNT_ALL & (_capi.RANGE_TO_DEST | _capi.OCCLUDE_ANY_OPAQUE) == 0
    assert callable(R.Scene.multi_hit_device)


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include "raytracert.h"\n' + PROTO +
                   "typedef char k_max[RT_MULTI_HIT_MAX == 16 ? 1 : -1];\n"
                   "unsigned flags(void) { return RT_RANGE_TO_DEST | RT_MULTI_COUNT_ALL; }\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cxx_forwarder_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "f.cpp"
    src.write_text('#include "raytracert.hpp"\n'
                   "void f(rtamd::RayTracer &s, const void *o, const void *d, void *hits, void *nhits) {\n"
                   "    s.multi_hit_range_device(o, d, RT_RAYS_PACKED, 8, nullptr, nullptr, nullptr, RT_MULTI_COUNT_ALL, 4, hits, nhits, nullptr); }\n")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "f.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _call(scene, n=4, stride=3, a=0x1000, b=0x2000, count=None, tmin=None, tmax=None, flags=0, k=4, out=0x3000, nhits=0x4000):
    """The entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    h = scene.handle if scene is not None else None
    vp = lambda x: None if x is None else C.c_void_p(x)
    return _capi.lib().rt_multi_hit_range_device(h, vp(a), vp(b), stride, n, vp(count), vp(tmin), vp(tmax), flags, k, vp(out),
                                                 vp(nhits), None)


ARG_CASES = {
    "n < 0": dict(n=-1),
    "stride": dict(stride=5),
    "null rays": dict(b=None),
    "padded rays not 16-byte aligned": dict(stride=4, a=0x1004),
    "d_count not 4-byte aligned": dict(count=0x5002),
    "d_tmin not 4-byte aligned": dict(tmin=0x6001),
    "d_tmax not 4-byte aligned": dict(tmax=0x7002),
    "unknown flag bit": dict(flags=1 << 3),
    "unknown high flag bit": dict(flags=(1 << 31) | 1),
    "a flag the entry does not use": dict(flags=_capi.OCCLUDE_ANY_OPAQUE),
    "k = 0": dict(k=0),
    "k < 0": dict(k=-3),
    "k above the largest": dict(k=_capi.MULTI_HIT_MAX + 1),
    "null hits": dict(out=None),
    "hits not 16-byte aligned": dict(out=0x3008),
    "nhits not 4-byte aligned": dict(nhits=0x4002),
    "count-all without nhits": dict(flags=_capi.MULTI_COUNT_ALL, nhits=None),
    "n * k above INT32_MAX": dict(n=2 ** 31 - 1, k=2),
}


def test_null_scene_is_an_argument_error():
    assert _call(None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()
    for what, kw in ARG_CASES.items():
        assert _call(None, **kw) == _capi.RT_E_ARG, what


def test_host_only_scene_has_no_device(host_scene):
    assert _call(host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    for what, kw in ARG_CASES.items():                       # ... and that is checked before every other argument
        assert _call(host_scene, **kw) == _capi.RT_E_NODEV, what
    assert _call(host_scene, n=0) == _capi.RT_E_NODEV


def test_python_method_refuses_bad_arguments_before_any_device(host_scene):
    import torch
    good = torch.zeros((5, 3), dtype=torch.float32)
    bad = {
        "numpy": np.zeros((5, 3), np.float32),
        "cpu tensor": good,
        "float64": torch.zeros((5, 3), dtype=torch.float64),
        "shape (n, 2)": torch.zeros((5, 2), dtype=torch.float32),
        "non-contiguous": torch.zeros((5, 6), dtype=torch.float32)[:, ::2],
    }
    for what, x in bad.items():
        with pytest.raises(ValueError):
            host_scene.multi_hit_device(x, good, 4)
        with pytest.raises(ValueError):
            host_scene.multi_hit_device(good, x, 4)
    with pytest.raises(ValueError, match="intersect_mesh"):   # the message points to the host method
        host_scene.multi_hit_device(bad["numpy"], bad["numpy"], 1)


def test_python_method_checks_k(host_scene):
    import torch
    good = torch.zeros((5, 3), dtype=torch.float32)
    for k in (0, -1, _capi.MULTI_HIT_MAX + 1, 2.0, None, True):
        with pytest.raises(ValueError, match="k must be"):
            host_scene.multi_hit_device(good, good, k)
