"""The device-resident query entries (rt_intersect_mesh_device, rt_occluded_device, rt_trace_rays_device)
without a GPU: exported and declared, the header still C, and every argument check that comes before a
device is touched, in the C ABI and in the Python methods."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracert_amd as R
from raytracert_amd import _capi

ENTRIES = ("rt_intersect_mesh_device", "rt_occluded_device", "rt_trace_rays_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    p = tmp_path_factory.mktemp("dq") / "t.obj"
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
    assert "#define RT_RAYS_PACKED 3" in text and "#define RT_RAYS_PADDED 4" in text
    assert (_capi.RAYS_PACKED, _capi.RAYS_PADDED) == (3, 4)


def test_header_still_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "h.c"
    src.write_text('#include "raytracert.h"\n'
                   "int (*const f0)(rt_scene *, const void *, const void *, int32_t, int32_t, const void *, void *, void *, void *)"
                   " = rt_intersect_mesh_device;\n"
                   "int (*const f1)(rt_scene *, const void *, const void *, int32_t, int32_t, const void *, void *, void *)"
                   " = rt_occluded_device;\n"
                   "int (*const f2)(rt_scene *, const rt_params *, const void *, const void *, int32_t, int32_t, void *, void *,"
                   " uint64_t *) = rt_trace_rays_device;\n"
                   "int stride_sum(void) { return RT_RAYS_PACKED + RT_RAYS_PADDED; }\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _call(name, scene, n=4, stride=3, a=0x1000, b=0x2000, out=0x3000, out2=0x4000, count=None, params=None):
    """One entry with made-up device addresses (never dereferenced: every case here is refused first)."""
    lib = _capi.lib()
    h = scene.handle if scene is not None else None
    vp = lambda x: None if x is None else C.c_void_p(x)
    if name == "rt_intersect_mesh_device":
        return lib.rt_intersect_mesh_device(h, vp(a), vp(b), stride, n, vp(count), vp(out), vp(out2), None)
    if name == "rt_occluded_device":
        return lib.rt_occluded_device(h, vp(a), vp(b), stride, n, vp(count), vp(out), None)
    p = params if params is not None else R.RenderParams(width=4, height=4, pf=1, max_lvl=1).to_c()
    return lib.rt_trace_rays_device(h, C.byref(p), vp(a), vp(b), stride, n, vp(out), None, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_null_scene_is_an_argument_error(name):
    assert _call(name, None) == _capi.RT_E_ARG
    assert _capi.lib().rt_last_error_string()


@pytest.mark.parametrize("name", ENTRIES)
def test_host_only_scene_has_no_device(name, host_scene):
    assert _call(name, host_scene) == _capi.RT_E_NODEV
    assert len(_capi.lib().rt_last_error_string()) > 0
    # ... and that is checked before the other arguments, as rt_intersect_mesh does
    assert _call(name, host_scene, n=-1, stride=7, a=None) == _capi.RT_E_NODEV


def test_python_methods_refuse_host_data_before_any_device(host_scene):
    import torch
    P = R.RenderParams(width=4, height=4, pf=1, max_lvl=1)
    good = torch.zeros((5, 3), dtype=torch.float32)
    calls = [lambda o, d: host_scene.intersect_mesh_device(o, d),
             lambda o, d: host_scene.occluded_device(o, d),
             lambda o, d: host_scene.perform_ray_tracing_device(P, o, d)]
    bad = {
        "numpy": np.zeros((5, 3), np.float32),
        "cpu tensor": good,
        "float64": torch.zeros((5, 3), dtype=torch.float64),
        "shape (n, 2)": torch.zeros((5, 2), dtype=torch.float32),
        "non-contiguous": torch.zeros((5, 6), dtype=torch.float32)[:, ::2],
    }
    assert not bad["non-contiguous"].is_contiguous() and bad["non-contiguous"].shape == (5, 3)
    for call in calls:
        for what, x in bad.items():
            with pytest.raises(ValueError):
                call(x, good)
            with pytest.raises(ValueError):
                call(good, x)
    with pytest.raises(ValueError, match="intersect_mesh"):   # the message points to the host method
        host_scene.intersect_mesh_device(bad["numpy"], bad["numpy"])
    with pytest.raises(ValueError, match="perform_ray_tracing"):
        host_scene.perform_ray_tracing_device(P, good, good)
