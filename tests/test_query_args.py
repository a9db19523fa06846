"""The device-resident query entries' argument rules on the host (raytracert_amd/csrc/query_args.h, the header
rt_capi.cpp refuses a call by, built by g++ without HIP): per entry a call in order, every rule broken alone and
its message, the order of the rules (of two adjacent ones the earlier wins; with all broken, the first), and
n == 0 (null arrays pass, the rules that do not depend on n still hold) (tests/cxx/query_args_check.cpp). Which
rule fires first is only visible through the C ABI on a device scene; here it needs no GPU. The program is also
run built with the host sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The query section of rt_capi.cpp, as it stood before the header, had 82 rule lines (`return fail(RT_E_ARG, ...)`
# from check_device_rays to the end of rt_triangle_collides_device, without rt_closest_point's, which takes host
# arrays). 28 of them stood in helpers that several entries shared: the four check_device_* of 5 lines each (rays
# in 5 entries, points in 5, boxes in 2, triangles in 2), check_range_args' 3 in 3 entries and check_point_args' own
# 5 in 2. The other 54 stood in the entries. Counted once per entry that applied them that makes
# 54 + 5 * (5 + 5 + 2 + 2) + 3 * 3 + 5 * 2 = 143: per entry, in the header's order,
# 7 + 7 + 11 + 9 + 14 + 10 + 14 + 8 + 10 + 11 + 13 + 8 + 13 + 8.
RULES = 143


def _build(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I" + os.path.join(ROOT, "raytracert_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "query_args_check.cpp"), "-o", out], check=True)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-4000:] + r.stderr[-4000:]
    return int(r.stdout.split()[1])


def test_query_args_rules(tmp_path):
    exe = str(tmp_path / "query_args_check")
    _build(exe)
    assert _run(exe) == RULES   # (no entry and no rule skipped)


def test_query_args_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "query_args_check_san")
    try:
        _build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build the stand-alone check with -fsanitize=address,undefined")
    assert _run(exe) == RULES
