#!/usr/bin/env python3
"""What the closest-point device query costs (DESIGN.md "Closest-point queries"). On C4 (102,402 triangles), for
two point sets,

* uniform: 1,000,000 points uniform in the scene's box (default_rng(11)),
* surface: the hit points of the 2,073,600 primary rays of the default 1920x1080 view, pushed 0.01 along their
  face normals (coherent, near the surface),

it times, in one run per point set, each as the median of 20 GPU times between two events after 3 warm-ups (with
the fastest and slowest of the 20 as the spread):

* rt_closest_point_device on the trees of the three builders (SAH, LBVH, CLUSTER), four-wide and binary,
* the loop over every triangle (RT_ACCEL_BRUTE_FORCE) on the first 10,000 of the points,
* rt_closest_hit_range_device with NULL bounds on the same number of rays, for scale (uniform: random pairs of
  the points; surface: the primary rays themselves).

A second, untimed pass under RT_PROFILE_WORK counts the point-triangle evaluations and node visits per point.

The leg "qwork" records, for scene Q of the tests and the 256 in-box points of tests/_closest_point_ref.py, the
evaluations per point of every builder and width: the numbers tests/test_gpu_closest_point.py pins.

Each leg runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/closest_point_probe.py out.json [uniform|surface|qwork ...]   (results are merged into out.json)
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


def qwork(out_path):
    import numpy as np
    import torch

    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import raytracert_amd as R
    from raytracert_amd import _capi, scenes
    import _closest_point_ref as CP
    import _query_scenes as QS

    dev = torch.device("cuda", 0)
    path = scenes.write_sphere_grid(QS.SPEC_Q, tempfile.mkdtemp(), "cp_q")
    with R.Scene.load(path, device=0) as sc:
        e = sc.export()
        T = np.ascontiguousarray(e["vertices"][e["triangles"].astype(np.int64)], np.float32)
        p = CP.in_box_points(T)
        dp = torch.from_numpy(p).to(dev)
        r = dict(triangles=len(T), points=len(p))
        sc.set_profiling(True, count_work=True)
        for b in BUILDERS:
            sc.set_builder(b)
            sc.update_vertices(e["vertices"], "rebuild")
            r[b] = {}
            for width in (4, 2):
                sc.tune("bvh_width", width)
                sc.reset_stats()
                sc.closest_point_device(dp)
                torch.cuda.synchronize(dev)
                t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                r[b][f"width{width}"] = dict(evaluations_per_point=round(t / len(p), 3), node_visits_per_point=round(v / len(p), 3))
        sc.set_profiling(False)
    print("qwork", json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(r, f)


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
            hits = int((tri >= 0).sum().item())
        else:
            rng = np.random.default_rng(11)
            lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
            pts = torch.from_numpy(rng.uniform(lo, hi, (1_000_000, 3)).astype(np.float32)).to(dev)
            o3, d3 = pts, pts.roll(1, 0).contiguous()
            hits = None
        n = len(pts)
        rec1 = torch.empty((n, 4), dtype=torch.int32, device=dev)
        recb = torch.empty((N_BRUTE, 4), dtype=torch.int32, device=dev)
        pb = pts[:N_BRUTE].contiguous()

        def query():
            return sc.closest_point_device(pts, out=rec1)

        def brute():
            return sc.closest_point_device(pb, out=recb)

        def rays():
            return sc.closest_hit_device(o3, d3, out=rec1)

        r = dict(points=n, triangles=int(len(e["triangles"])))
        if hits is not None:
            r["primary_rays_that_hit"] = hits
        r["closest_hit_record_ms"] = event_ms(rays)
        ref = None
        for b in BUILDERS:
            sc.set_builder(b)
            sc.update_vertices(verts, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                key = f"{b}_width{width}"
                r[key + "_ms"] = event_ms(query)
                query()
                got = rec1.clone()
                ref = got if ref is None else ref
                r[key + "_same_bytes_as_first"] = bool(torch.equal(got, ref))
                sc.set_profiling(True, count_work=True)              # untimed: the counting instantiation
                sc.reset_stats()
                query()
                torch.cuda.synchronize(dev)
                t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                sc.set_profiling(False)
                r[key + "_work"] = dict(evaluations_per_point=round(t / n, 3), node_visits_per_point=round(v / n, 3))
                r[key + "_ns_per_point"] = round(r[key + "_ms"]["median"] * 1e6 / n, 3)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        r[f"brute_force_{N_BRUTE}_points_ms"] = event_ms(brute)
        brute()
        r["brute_force_same_bytes_as_first"] = bool(torch.equal(recb, ref[:N_BRUTE]))
        r["brute_force_ns_per_point"] = round(r[f"brute_force_{N_BRUTE}_points_ms"]["median"] * 1e6 / N_BRUTE, 3)
        r["brute_force_evaluations_per_point"] = r["triangles"]
        sc.set_accel("bvh")
        r["ratio_brute_over_sah_width4_per_point"] = round(r["brute_force_ns_per_point"] / r["sah_width4_ns_per_point"], 1)
        r["ratio_sah_width4_over_closest_hit_record"] = round(r["sah_width4_ms"]["median"] / r["closest_hit_record_ms"]["median"], 3)
    print(name, json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(r, f)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    names = sys.argv[2:] or ["uniform", "surface", "qwork"]
    results = {}
    for name in names:                                           # a fresh process per leg, each under its own limit
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
        doc = dict(probe="tools/closest_point_probe.py", scene="C4 (102,402 triangles)",
                   runs="median (min, max) of 20 GPU times between events after 3 warm-ups; work: untimed counting pass", point_sets={})
        if os.path.exists(out_path):
            with open(out_path) as f:
                doc = json.load(f)
        if "qwork" in results:
            doc["scene_q_work"] = results.pop("qwork")
        doc["point_sets"].update(results)
        with open(out_path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        qwork(sys.argv[3]) if sys.argv[2] == "qwork" else one(sys.argv[2], sys.argv[3])
    else:
        main()
