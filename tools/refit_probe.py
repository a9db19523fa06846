#!/usr/bin/env python3
"""What an animated mesh costs (dynamic geometry, DESIGN.md "Dynamic geometry"): for C4 and C5 under the
deformation D(a) (x += a sin(7y + 1), z += a cos(5x), a up to 0.01),

* the time of one rt_scene_update_vertices call (host array) and one rt_scene_update_vertices_device call
  (device array): median of 50 after 5 warm-up updates, by the host's wall clock around the call and by a
  pair of device events recorded on the caller's stream around it (the call returns with the update
  complete, so the two agree up to the launch latency);
* on the same run, the only alternative without the entry: rt_scene_destroy + rt_scene_create with the
  same arrays, median of 5;
* the frame time, one frame at a time, after the 50 accumulated refits, and after mode="rebuild" of the
  same vertices: their ratio says when to ask for RT_UPDATE_REBUILD.

Usage: python tools/refit_probe.py [out.json] [workload ...]   (default: c4 c5)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import bench  # noqa: E402
import raytracert_amd as R  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
names = sys.argv[2:] or ["c4", "c5"]
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)


def deform(v, a):
    v = np.array(v, np.float32)
    a = np.float32(a)
    x, y = v[:, 0].copy(), v[:, 1]
    v[:, 0] = x + a * np.sin(np.float32(7) * y + np.float32(1))
    v[:, 2] = v[:, 2] + a * np.cos(np.float32(5) * x)
    return v


def timed(fn):
    """(wall ms, event ms) of fn(), from an idle device."""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    e1.record(st)
    torch.cuda.synchronize(dev)
    return wall, e0.elapsed_time(e1)


def med(rows):
    a = np.array(rows)
    return [round(float(x), 4) for x in np.median(a, axis=0)]


results = {}
for name in names:
    wl = bench.WORKLOADS[name]
    W, H = wl["width"], wl["height"]
    path = bench.workload_scene(wl["scene"], tempfile.mkdtemp())
    p = R.RenderParams(width=W, height=H, pf=wl["pf"], max_lvl=wl["max_lvl"], lights=[list(x) for x in wl["lights"]]).to_c()
    buf = torch.zeros(H * W * 3, dtype=torch.uint8, device=dev)

    def frame_ms(sc, warm=40, n=50):
        def one():
            sc.render_frame_device(p, 16, 16, buf.data_ptr(), buf.numel(), st.cuda_stream)
            torch.cuda.synchronize(dev)
        for _ in range(warm):
            one()
        return med([timed(one) for _ in range(n)])[0]

    with R.Scene.load(path, device=0) as sc:
        e = sc.export()
        base = e["vertices"]
        steps = [deform(base, 0.01 * (1 + k % 5) / 5) for k in range(5)]   # (the last: D(0.01))
        dsteps = [torch.from_numpy(v).to(dev) for v in steps]
        r = dict(triangles=int(len(e["triangles"])), vertices=int(len(base)), frame_ms_static=frame_ms(sc))
        outcomes = set()
        for k in range(5):
            outcomes.add(sc.update_vertices(steps[k]))
        r["update_host_ms_wall_event"] = med([timed(lambda k=k: outcomes.add(sc.update_vertices(steps[k % 5]))) for k in range(50)])
        for k in range(5):
            outcomes.add(sc.update_vertices(dsteps[k]))
        r["update_device_ms_wall_event"] = med([timed(lambda k=k: outcomes.add(sc.update_vertices(dsteps[k % 5]))) for k in range(50)])
        r["outcomes"] = sorted(outcomes)
        r["frame_ms_after_refits"] = frame_ms(sc)
        refit_frame = buf.cpu().numpy().copy()
        r["rebuild_ms_wall_event"] = med([timed(lambda: outcomes.add(sc.update_vertices(steps[4], mode="rebuild")))])
        r["frame_ms_after_rebuild"] = frame_ms(sc)
        r["frames_equal"] = bool(np.array_equal(refit_frame, buf.cpu().numpy()))
    # the alternative: destroy + create with the same arrays
    rows = []
    sc = R.Scene.create(base, e["triangles"], e["tri_mat"], e["materials"], device=0)
    for k in range(5):
        def recreate(k=k):
            global sc
            sc.close()
            sc = R.Scene.create(steps[k], e["triangles"], e["tri_mat"], e["materials"], device=0)
        rows.append(timed(recreate))
    sc.close()
    r["recreate_ms_wall_event"] = med(rows)
    r["update_over_frame"] = round(r["update_host_ms_wall_event"][0] / r["frame_ms_static"], 3)
    r["update_device_over_frame"] = round(r["update_device_ms_wall_event"][0] / r["frame_ms_static"], 3)
    r["recreate_over_update"] = round(r["recreate_ms_wall_event"][0] / r["update_host_ms_wall_event"][0], 1)
    r["refit_frame_over_rebuilt_frame"] = round(r["frame_ms_after_refits"] / r["frame_ms_after_rebuild"], 4)
    results[name] = r
    print(name, json.dumps(r), flush=True)

text = json.dumps(dict(probe="tools/refit_probe.py", deformation="D(a): x += a sin(7y + 1), z += a cos(5x), a in 0.002..0.01",
                       workloads=results), indent=1)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
