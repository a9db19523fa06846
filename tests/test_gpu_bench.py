"""A plain bench.py run (one GPU, no --full): it times exactly --steps steps, prints the headline alone
and, with --dump-outputs, writes the frames of its last timed call, which must be the library's
renders of those camera-path views.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import raytracert_amd as R
from _util import ROOT, scene_path
from raytracert_amd import scenes

pytestmark = pytest.mark.gpu

W, H = 800, 600   # bench.py's C2 workload: dodgeColorTest.obj, pf 1, depth 1, one light


def test_plain_run_headline_and_dumped_frames(workdir, tmp_path, gpu_available):
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--workload", "c2", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["n_gpus"] == 1
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert d["config"]["frames_per_call"] == 8 and d["config"]["value_mode"] == "8_frames_per_call_camera_path"
    # the legs of --full did not run
    for k in ("roofline", "kernel_ms_per_step", "cpu_baseline", "strong_shares", "shard_path", "batches"):
        assert k not in d
    for k in ("one_in_flight", "orbit", "multi_frame", "first_frame_ms", "end_to_end"):
        assert k not in d["config"]
    assert sorted(os.listdir(dump)) == ["call_frames.npy", "frame.npy"]
    frame, call = np.load(dump / "frame.npy"), np.load(dump / "call_frames.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3)
    assert call.dtype == np.float32 and call.shape == (3, H, W, 3)   # one call of the 3 timed frames
    assert np.array_equal(call[-1], frame)
    # the warm-up call rendered path views 0-7, the timed call 8, 9, 10: the default view turned by
    # 0, -0.25, -0.5 degrees (bench.py's triangle wave of period 16, step 0.25)
    rays = 0
    with R.Scene.load(scene_path("ref:dodgeColorTest.obj", workdir), device=0) as sc:
        for k, t in enumerate((0, -1, -2)):
            p = R.RenderParams(width=W, height=H, pf=1, max_lvl=1, lights=[(0.0, 0.0, 4.0)],
                               corners=scenes.orbit_corners(W, H, t, 0.25))
            u8, _, counts = sc.render(p)
            assert np.array_equal(call[k], u8.astype(np.float32)), f"timed frame {k}"
            rays += int(sum(int(c) for c in counts))
    assert len({call[k].tobytes() for k in range(3)}) == 3   # distinct views
    # value and ms_per_step describe the same three frames (both rounded in the line)
    assert d["value"] == pytest.approx(rays / 3 / (d["ms_per_step"] * 1e-3) / 1e6, rel=0.02)
