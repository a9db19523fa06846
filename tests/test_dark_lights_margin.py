"""The dark-light rule's margin on the host (raytracert_amd/csrc/dark_lights.h, the header the chain kernels
use, built by g++ with -ffp-contract=off): over 10^7 random (normal, point, camera, light) tuples and 1.3
million adversarial ones (facing cosines within parts in a thousand of the margin on both sides, the light
opposite the camera, distances from 1e-18 to 3e19, normals too short to normalise), whenever the rule says
dark, both of shade_hit's terms are exact zeros in binary32, their dot products are negative, and the
normal after the light's in-place normalisations is the stored normal bit for bit
(tests/cxx/dark_lights_check.cpp). The program is also run built with the host sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra,
                    "-I" + os.path.join(ROOT, "raytracert_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "dark_lights_check.cpp"), "-o", out, "-lm"], check=True)


def _run(exe, n):
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    return [int(x) for x in r.stdout.split()[1:4]]


def test_rule_says_dark_only_where_both_terms_are_zero(tmp_path):
    exe = str(tmp_path / "dark_lights_check")
    _build(exe)
    tuples, dark, near = _run(exe, 10_000_000)
    assert tuples >= 11_000_000
    # the check is not vacuous: the rule fires on random tuples and on tuples at the margin
    assert dark >= 100_000 and near >= 10_000, (tuples, dark, near)


def test_rule_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "dark_lights_check_san")
    try:
        _build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build the stand-alone check with -fsanitize=address,undefined")
    _run(exe, 300_000)
