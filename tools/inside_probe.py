#!/usr/bin/env python3
"""What the inside and signed-distance device queries cost (DESIGN.md "Inside and signed-distance queries"). On C4
(102,402 triangles), for the closest-point probe's two point sets,

* uniform: 1,000,000 points uniform in the scene's box (default_rng(11)),
* surface: the hit points of the 2,073,600 primary rays of the default 1920x1080 view, pushed 0.01 along their
  face normals (coherent, near the surface),

it times, in one run per point set, each as the median of 20 GPU times between two events after 3 warm-ups (with
the fastest and slowest of the 20 as the spread), along +z:

* rt_point_inside_device on the trees of the three builders (SAH, LBVH, CLUSTER), four-wide and binary,
* rt_closest_point_device and rt_signed_distance_device on the same trees (the second is the first's launch
  followed by the inside launch),
* rt_multi_hit_range_device with k = 1 and RT_MULTI_COUNT_ALL on rays from the points along +z, the way to a
  parity before this query (wrong under shared edges),
* the loop over every triangle (RT_ACCEL_BRUTE_FORCE) on the first 10,000 of the points.

A second, untimed pass under RT_PROFILE_WORK counts the triangle evaluations and node visits per point.

Each point set runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/inside_probe.py out.json [uniform|surface ...]   (results are merged into out.json)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 300
WARM, N = 3, 20
BUILDERS = ("sah", "lbvh", "cluster")
N_BRUTE = 10_000
AXIS = 4   # +z


def one(name, out_path):
    import numpy as np
    import torch

    sys.path.insert(0, HERE)
    import bench
    import raytracert_amd as R
    from raytracert_amd import _capi

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)

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

    wl = bench.WORKLOADS["c4"]
    path = bench.workload_scene(wl["scene"], tempfile.mkdtemp())
    with R.Scene.load(path, device=0) as sc:
        e = sc.export()
        verts = e["vertices"]
        if name == "surface":
            p = R.RenderParams(width=wl["width"], height=wl["height"], pf=1, max_lvl=0, lights=[list(x) for x in wl["lights"]])
            rec, _ = sc.trace_frame_samples(p, with_rays=True)
            rec = rec.reshape(-1, 9)
            o3 = torch.from_numpy(np.ascontiguousarray(rec[:, 0:3])).to(dev)
            d3 = torch.from_numpy(np.ascontiguousarray(rec[:, 3:6])).to(dev)
            tri, _, _, hit = sc.closest_hit_device(o3, d3, want_points=True)
            nrm = torch.from_numpy(np.ascontiguousarray(e["normals"], np.float32)).to(dev)
            pts = (hit + 0.01 * nrm[tri.clamp(min=0).long()]).contiguous()      # (a miss: the point (0,0,0) + a normal)
        else:
            rng = np.random.default_rng(11)
            lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
            pts = torch.from_numpy(rng.uniform(lo, hi, (1_000_000, 3)).astype(np.float32)).to(dev)
        n = len(pts)
        up = pts.clone()
        up[:, 2] += 1.0                                                         # the rays of the hit-count route
        ins = torch.empty((n,), dtype=torch.uint8, device=dev)
        cr = torch.empty((n,), dtype=torch.int32, device=dev)
        rec1 = torch.empty((n, 4), dtype=torch.int32, device=dev)
        recm = torch.empty((n, 1, 4), dtype=torch.int32, device=dev)
        nh = torch.empty((n,), dtype=torch.int32, device=dev)
        pb = pts[:N_BRUTE].contiguous()
        insb = torch.empty((N_BRUTE,), dtype=torch.uint8, device=dev)
        crb = torch.empty((N_BRUTE,), dtype=torch.int32, device=dev)

        def inside():
            return sc.point_inside_device(pts, axis=AXIS, crossings=True, out=(ins, cr))

        def closest():
            return sc.closest_point_device(pts, out=rec1)

        def signed():
            return sc.signed_distance_device(pts, axis=AXIS, out=rec1)

        def counted():
            return sc.multi_hit_device(pts, up, 1, count_all=True, out=(recm, nh))

        def brute():
            return sc.point_inside_device(pb, axis=AXIS, crossings=True, out=(insb, crb))

        r = dict(points=n, triangles=int(len(e["triangles"])), axis="+z")
        ref = None
        for b in BUILDERS:
            sc.set_builder(b)
            sc.update_vertices(verts, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                key = f"{b}_width{width}"
                r[key + "_closest_point_ms"] = event_ms(closest)
                r[key + "_inside_ms"] = event_ms(inside)
                r[key + "_signed_distance_ms"] = event_ms(signed)
                r[key + "_multi_hit_count_all_ms"] = event_ms(counted)
                inside()
                got = cr.clone()
                if ref is None:
                    ref = got
                    counted()
                    r["inside_fraction"] = round(float(ins.float().mean().item()), 4)
                    r["points_where_hit_count_parity_differs"] = int(((nh & 1) != ins.to(torch.int32)).sum().item())
                r[key + "_same_crossings_as_first"] = bool(torch.equal(got, ref))
                sc.set_profiling(True, count_work=True)              # untimed: the counting instantiation
                sc.reset_stats()
                inside()
                torch.cuda.synchronize(dev)
                t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                sc.set_profiling(False)
                r[key + "_inside_work"] = dict(evaluations_per_point=round(t / n, 3), node_visits_per_point=round(v / n, 3))
                cp = r[key + "_closest_point_ms"]["median"]
                r[key + "_inside_over_closest_point"] = round(r[key + "_inside_ms"]["median"] / cp, 3)
                r[key + "_signed_distance_over_closest_point"] = round(r[key + "_signed_distance_ms"]["median"] / cp, 3)
                r[key + "_multi_hit_count_all_over_closest_point"] = round(r[key + "_multi_hit_count_all_ms"]["median"] / cp, 3)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        r[f"brute_force_{N_BRUTE}_points_ms"] = event_ms(brute)
        brute()
        r["brute_force_same_crossings_as_first"] = bool(torch.equal(crb, ref[:N_BRUTE]))
        r["brute_force_ns_per_point"] = round(r[f"brute_force_{N_BRUTE}_points_ms"]["median"] * 1e6 / N_BRUTE, 3)
        sc.set_accel("bvh")
    print(name, json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(r, f)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    names = sys.argv[2:] or ["uniform", "surface"]
    results = {}
    for name in names:                                           # a fresh process per point set, each under its own limit
        part = os.path.join(tempfile.mkdtemp(), name + ".json")
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, part], timeout=STEP_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {STEP_LIMIT_S} s; nothing further is started")
        if rc != 0:
            sys.exit(f"{name}: exit status {rc}; nothing further is started")
        with open(part) as f:
            results[name] = json.load(f)
    if out_path:
        doc = dict(probe="tools/inside_probe.py", scene="C4 (102,402 triangles)",
                   runs="median (min, max) of 20 GPU times between events after 3 warm-ups; work: untimed counting pass", point_sets={})
        if os.path.exists(out_path):
            with open(out_path) as f:
                doc = json.load(f)
        doc["point_sets"].update(results)
        with open(out_path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
    else:
        main()
