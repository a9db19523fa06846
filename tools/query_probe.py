#!/usr/bin/env python3
"""What a batch of ray queries costs when the rays are born on the GPU (DESIGN.md "Device-resident
queries"). On C4 (102,402 triangles), for two ray sets,

* primary: the 2,073,600 primary rays of the default 1920x1080 view (as the device makes them:
  rt_trace_frame_samples' ray records),
* random:  1,000,000 pairs of standard-normal points x 0.5 (incoherent rays through the scene),

it times, each as the median of 20 after 3 warm-ups (with the fastest and slowest of the 20 as the spread):

(a) rt_intersect_mesh with host arrays: wall time of the call (repack, two uploads, kernel, two downloads);
(b) rt_intersect_mesh_device with device tensors: wall time of the call plus one stream synchronisation;
(c) its GPU time between two events, rays packed (stride 3) and padded (stride 4);
(d) rt_occluded_device's GPU time on C4 (no transparent material: the any-hit walk) and on C4's grid with
    the F4 fixtures' transparent material (closest hit, then the material's test).

Usage: python tools/query_probe.py out.json [primary|random ...]   (results are merged into out.json)
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
from raytracert_amd import scenes  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
names = sys.argv[2:] or ["primary", "random"]
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
WARM, N = 3, 20


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def wall_ms(fn):
    for _ in range(WARM):
        fn()
    rows = []
    for _ in range(N):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        rows.append((time.perf_counter() - t0) * 1e3)
    return stats(rows)


def event_ms(fn):
    for _ in range(WARM):
        fn()
    rows = []
    for _ in range(N):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        rows.append(e0.elapsed_time(e1))
    return stats(rows)


def ray_set(name, sc, wl):
    if name == "primary":
        p = R.RenderParams(width=wl["width"], height=wl["height"], pf=1, max_lvl=0, lights=[list(x) for x in wl["lights"]])
        rec, _ = sc.trace_frame_samples(p, with_rays=True)
        rec = rec.reshape(-1, 9)
        return np.ascontiguousarray(rec[:, 0:3]), np.ascontiguousarray(rec[:, 3:6])
    rng = np.random.default_rng(11)
    n = 1_000_000
    return ((rng.standard_normal((n, 3)) * 0.5).astype(np.float32), (rng.standard_normal((n, 3)) * 0.5).astype(np.float32))


def padded(a):
    return torch.from_numpy(np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1)).to(dev)


results = {}
wl = bench.WORKLOADS["c4"]
work = tempfile.mkdtemp()
path = bench.workload_scene(wl["scene"], work)
c4 = scenes.C4
tpath = scenes.write_sphere_grid(scenes.GridSpec(grid=c4.grid, slices=c4.slices, stacks=c4.stacks, spacing=c4.spacing,
                                                 radius=c4.radius, transparent=True), work, "c4_transparent")
with R.Scene.load(path, device=0) as sc, R.Scene.load(tpath, device=0) as tsc:
    for name in names:
        o, d = ray_set(name, sc, wl)
        n = len(o)
        o3, d3 = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        o4, d4 = padded(o), padded(d)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        blk = torch.empty(n, dtype=torch.uint8, device=dev)
        hidx, hpts = sc.intersect_mesh(o, d)
        sc.intersect_mesh_device(o4, d4, out=(idx, pts))
        r = dict(rays=n, hits=int((hidx >= 0).sum()),
                 device_equals_host=bool(np.array_equal(idx.cpu().numpy(), hidx) and
                                         np.array_equal(pts.cpu().numpy().view(np.uint32), hpts.view(np.uint32))))

        def device_call():
            sc.intersect_mesh_device(o3, d3, out=(idx, pts))
            st.synchronize()

        r["a_host_intersect_mesh_wall_ms"] = wall_ms(lambda: sc.intersect_mesh(o, d))
        r["b_device_intersect_mesh_wall_ms"] = wall_ms(device_call)
        r["c_device_gpu_ms_stride3"] = event_ms(lambda: sc.intersect_mesh_device(o3, d3, out=(idx, pts)))
        r["c_device_gpu_ms_stride4"] = event_ms(lambda: sc.intersect_mesh_device(o4, d4, out=(idx, pts)))
        r["d_occluded_gpu_ms_any_hit_c4"] = event_ms(lambda: sc.occluded_device(o3, d3, out=blk))
        r["blocked_c4"] = int(blk.sum().item())
        r["d_occluded_gpu_ms_closest_hit_transparent_grid"] = event_ms(lambda: tsc.occluded_device(o3, d3, out=blk))
        r["blocked_transparent_grid"] = int(blk.sum().item())
        r["host_over_device_wall"] = round(r["a_host_intersect_mesh_wall_ms"]["median"] / r["b_device_intersect_mesh_wall_ms"]["median"], 1)
        r["mrays_per_s_device_stride3"] = round(n / r["c_device_gpu_ms_stride3"]["median"] / 1e3, 1)
        results[name] = r
        print(name, json.dumps(r), flush=True)

if out_path:
    doc = dict(probe="tools/query_probe.py", scene="C4 (102,402 triangles)", runs="median (min, max) of 20 after 3 warm-ups", ray_sets={})
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc["ray_sets"].update(results)
    with open(out_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
