#!/usr/bin/env python3
"""What the ranged device queries cost next to the half-line ones (DESIGN.md "Ranged device queries"). On C4
(102,402 triangles) and on C4's grid with one transparent material, for two ray sets,

* primary: the 2,073,600 primary rays of the default 1920x1080 view,
* random:  1,000,000 pairs of standard-normal points x 0.5 (incoherent rays through the scene),

it times, in one run, each as the median of 20 GPU times between two events after 3 warm-ups (with the fastest
and slowest of the 20 as the spread):

(a) rt_intersect_mesh_device against rt_closest_hit_range_device with NULL bounds (records alone, and with the
    points: 16 or 28 bytes stored per ray against 16);
(b) rt_occluded_device against rt_occluded_range_device with RT_RANGE_TO_DEST under each rule, and with NULL
    bounds, on both scenes.

A second, untimed pass under RT_PROFILE_WORK counts the node visits and triangle tests of each (the counting
instantiations), which is what explains the ratios.

Usage: python tools/range_probe.py out.json [primary|random ...]   (results are merged into out.json)
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import bench  # noqa: E402
import raytracert_amd as R  # noqa: E402
from raytracert_amd import _capi, scenes  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
names = sys.argv[2:] or ["primary", "random"]
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
WARM, N = 3, 20


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 4), min=round(xs[0], 4), max=round(xs[-1], 4))


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


def work(scene, kind, fn):
    """(triangle tests, node visits) per ray of one call, by the counting instantiations."""
    scene.set_profiling(True, count_work=True)
    scene.reset_stats()
    fn()
    torch.cuda.synchronize(dev)
    t, v = scene.work_stats(kind)
    scene.set_profiling(False)
    return t, v


def ratio(r, a, b):
    return round(r[a]["median"] / r[b]["median"], 3)


results = {}
wl = bench.WORKLOADS["c4"]
tmp = tempfile.mkdtemp()
path = bench.workload_scene(wl["scene"], tmp)
c4 = scenes.C4
tpath = scenes.write_sphere_grid(scenes.GridSpec(grid=c4.grid, slices=c4.slices, stacks=c4.stacks, spacing=c4.spacing,
                                                 radius=c4.radius, transparent=True), tmp, "c4_transparent")
with R.Scene.load(path, device=0) as sc, R.Scene.load(tpath, device=0) as tsc:
    for name in names:
        o, d = ray_set(name, sc, wl)
        n = len(o)
        o3, d3 = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rec = torch.empty((n, 4), dtype=torch.int32, device=dev)
        rpts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        blk = torch.empty(n, dtype=torch.uint8, device=dev)
        sc.intersect_mesh_device(o3, d3, out=(idx, pts))
        sc.closest_hit_device(o3, d3, out=(rec, rpts), want_points=True)
        r = dict(rays=n, hits=int((idx >= 0).sum().item()),
                 null_bounds_equal_half_line=bool(torch.equal(rec[:, 0], idx) and
                                                  torch.equal(rpts.view(torch.int32), pts.view(torch.int32))))
        # (a) closest hit
        half = lambda: sc.intersect_mesh_device(o3, d3, out=(idx, pts))
        recs = lambda: sc.closest_hit_device(o3, d3, out=rec)
        recs_pts = lambda: sc.closest_hit_device(o3, d3, out=(rec, rpts), want_points=True)
        seg = lambda: sc.closest_hit_device(o3, d3, to_dest=True, out=rec)
        r["a_intersect_mesh_device_ms"] = event_ms(half)
        r["a_closest_record_null_bounds_ms"] = event_ms(recs)
        r["a_closest_record_and_point_null_bounds_ms"] = event_ms(recs_pts)
        r["a_closest_record_to_dest_ms"] = event_ms(seg)
        r["hits_to_dest"] = int((rec[:, 0] >= 0).sum().item())
        r["a_intersect_mesh_device_ms_again"] = event_ms(half)      # the baseline's own run-to-run spread
        r["ratio_record_over_half_line"] = ratio(r, "a_closest_record_null_bounds_ms", "a_intersect_mesh_device_ms")
        r["ratio_record_and_point_over_half_line"] = ratio(r, "a_closest_record_and_point_null_bounds_ms", "a_intersect_mesh_device_ms")
        r["ratio_record_to_dest_over_half_line"] = ratio(r, "a_closest_record_to_dest_ms", "a_intersect_mesh_device_ms")
        K = _capi.KERNEL_CLOSEST_HIT
        for key, fn in (("half_line", half), ("record_null_bounds", recs), ("record_to_dest", seg)):
            t, v = work(sc, K, fn)
            r["work_closest_" + key] = dict(tests_per_ray=round(t / n, 3), visits_per_ray=round(v / n, 3))
        # (b) occlusion, on C4 (nothing transparent: the any-hit walks) and on its transparent twin
        for tag, scene in (("c4", sc), ("transparent", tsc)):
            calls = {
                "occluded_device": lambda: scene.occluded_device(o3, d3, out=blk),
                "range_null_bounds": lambda: scene.occluded_range_device(o3, d3, out=blk),
                "range_null_bounds_any_opaque": lambda: scene.occluded_range_device(o3, d3, any_opaque=True, out=blk),
                "range_to_dest": lambda: scene.occluded_range_device(o3, d3, to_dest=True, out=blk),
                "range_to_dest_any_opaque": lambda: scene.occluded_range_device(o3, d3, to_dest=True, any_opaque=True, out=blk),
            }
            for key, fn in calls.items():
                r[f"b_{tag}_{key}_ms"] = event_ms(fn)
                r[f"blocked_{tag}_{key}"] = int(blk.sum().item())
                t, v = work(scene, _capi.KERNEL_SHADOW, fn)
                r[f"work_{tag}_{key}"] = dict(tests_per_ray=round(t / n, 3), visits_per_ray=round(v / n, 3))
            for key in list(calls)[1:]:
                r[f"ratio_{tag}_{key}_over_occluded_device"] = ratio(r, f"b_{tag}_{key}_ms", f"b_{tag}_occluded_device_ms")
        results[name] = r
        print(name, json.dumps(r), flush=True)

if out_path:
    doc = dict(probe="tools/range_probe.py", scene="C4 (102,402 triangles) and C4 with one transparent material",
               runs="median (min, max) of 20 GPU times between events after 3 warm-ups; work: untimed counting pass", ray_sets={})
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc["ray_sets"].update(results)
    with open(out_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
