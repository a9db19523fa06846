"""The chain launch policy on the host (raytracert_amd/csrc/launch_policy.h, the header rt_capi.cpp's run_chain
decides by, built by g++ without HIP): the trial tables, their key and launch schedule, the decision (warm-up
ignored, faster of two rounds, time per view, the 2% rule, the 3% and 15% rules of the in-flight and multi-frame
distributions), the fallback to the first candidate, adoption between pipelines, the batch order's life launch
by launch on a static and on a moving view, and the launch shape the knobs, the launch's facts and the trials
resolve to (tests/cxx/launch_policy_check.cpp). The program is also run built with the host sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I" + os.path.join(ROOT, "raytracert_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "launch_policy_check.cpp"), "-o", out], check=True)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-4000:] + r.stderr[-4000:]
    return int(r.stdout.split()[1])


def test_launch_policy_rules(tmp_path):
    exe = str(tmp_path / "launch_policy_check")
    _build(exe)
    assert _run(exe) >= 400   # (the check is not vacuous)


def test_launch_policy_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "launch_policy_check_san")
    try:
        _build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build the stand-alone check with -fsanitize=address,undefined")
    _run(exe)
