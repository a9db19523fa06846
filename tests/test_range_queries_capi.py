"""The ranged device queries (rt_closest_hit_range_device, rt_occluded_range_device) without a GPU: exported
and declared, the header still C with a 16-byte rt_hit, RT_E_NODEV on a host-only scene before any other check,
and the argument errors that can be reached without a device (a NULL scene refuses every call; the same cases on
a device scene, where each is the only thing wrong, are in tests/test_gpu_range_queries.py), in the C ABI and in
the Python methods."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

ENTRIES = ("rt_closest_hit_range_device", "rt_occluded_range_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("rq") / "t.obj"
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
    text = open(_capi.HEADER_PATH).read()
    assert "#define RT_RANGE_TO_DEST      (1u << 0)" in text and "#define RT_OCCLUDE_ANY_OPAQUE (1u << 1)" in text
    assert (_capi.RANGE_TO_DEST, _capi.OCCLUDE_ANY_OPAQUE, _capi.HIT_BYTES) == (1, 2, 16)
    for method in ("closest_hit_device", "occluded_range_device"):
        assert callable(getattr(R.Scene, method))


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "raytracert.h"\n'
                   "int (*const f0)(rt_scene *, const void *, const void *, int32_t, int32_t, const void *, const void *,"
                   " const void *, uint32_t, void *, void *, void *) = rt_closest_hit_range_device;\n"
                   "int (*const f1)(rt_scene *, const void *, const void *, int32_t, int32_t, const void *, const void *,"
                   " const void *, uint32_t, void *, void *) = rt_occluded_range_device;\n"
                   "typedef char hit_is_16_bytes[sizeof(rt_hit) == 16 ? 1 : -1];\n"
                   "typedef char hit_layout[offsetof(rt_hit, triangle) == 0 && offsetof(rt_hit, distance) == 4 &&"
                   " offsetof(rt_hit, s) == 8 && offsetof(rt_hit, t) == 12 ? 1 : -1];\n"
                   "unsigned flags(void) { return RT_RANGE_TO_DEST | RT_OCCLUDE_ANY_OPAQUE; }\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _call(name, scene, n=4, stride=3, a=0x1000, b=0x2000, count=None, tmin=None, tmax=None, flags=0, out=0x3000, out2=None):
    """One entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    lib = _capi.lib()
    h = scene.handle if scene is not None else None
    vp = lambda x: None if x is None else C.c_void_p(x)
    if name == "rt_closest_hit_range_device":
        return lib.rt_closest_hit_range_device(h, vp(a), vp(b), stride, n, vp(count), vp(tmin), vp(tmax), flags, vp(out), vp(out2), None)
    return lib.rt_occluded_range_device(h, vp(a), vp(b), stride, n, vp(count), vp(tmin), vp(tmax), flags, vp(out), None)


# the RT_E_ARG cases of the entries (include/raytracert.h), as keyword changes of a call that is otherwise in order
ARG_CASES = {
    "n < 0": dict(n=-1),
    "stride": dict(stride=5),
    "null rays": dict(b=None),
    "padded rays not 16-byte aligned": dict(stride=4, a=0x1004),
    "null output": dict(out=None),
    "d_count not 4-byte aligned": dict(count=0x5002),
    "d_tmin not 4-byte aligned": dict(tmin=0x6001),
    "d_tmax not 4-byte aligned": dict(tmax=0x7002),
    "unknown flag bit": dict(flags=1 << 2),
    "unknown high flag bit": dict(flags=(1 << 31) | 1),
}
CLOSEST_ONLY = {
    "d_hit_out not 16-byte aligned": dict(out=0x3008),
    "d_point_out not 4-byte aligned": dict(out2=0x4002),
    "a flag the entry does not use": dict(flags=_capi.OCCLUDE_ANY_OPAQUE),
}


def arg_cases(name):
    cases = dict(ARG_CASES)
    if name == "rt_closest_hit_range_device":
        cases.update(CLOSEST_ONLY)
    return cases


@pytest.mark.parametrize("name", ENTRIES)
def test_null_scene_is_an_argument_error(name):
    assert _call(name, None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()
    for what, kw in arg_cases(name).items():
        assert _call(name, None, **kw) == _capi.RT_E_ARG, what


@pytest.mark.parametrize("name", ENTRIES)
def test_host_only_scene_has_no_device(name, host_scene):
    assert _call(name, host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    # ... and that is checked before every other argument
    for what, kw in arg_cases(name).items():
        assert _call(name, host_scene, **kw) == _capi.RT_E_NODEV, what
    assert _call(name, host_scene, n=0) == _capi.RT_E_NODEV


def test_python_methods_refuse_bad_arguments_before_any_device(host_scene):
    import torch
    good = torch.zeros((5, 3), dtype=torch.float32)
    calls = [lambda o, d, **kw: host_scene.closest_hit_device(o, d, **kw),
             lambda o, d, **kw: host_scene.occluded_range_device(o, d, **kw)]
    bad = {
        "numpy": np.zeros((5, 3), np.float32),
        "cpu tensor": good,
        "float64": torch.zeros((5, 3), dtype=torch.float64),
        "shape (n, 2)": torch.zeros((5, 2), dtype=torch.float32),
        "non-contiguous": torch.zeros((5, 6), dtype=torch.float32)[:, ::2],
    }
    for call in calls:
        for what, x in bad.items():
            with pytest.raises(ValueError):
                call(x, good)
            with pytest.raises(ValueError):
                call(good, x)
    with pytest.raises(ValueError, match="intersect_mesh"):   # the message points to the host method
        host_scene.closest_hit_device(bad["numpy"], bad["numpy"])
