#!/usr/bin/env python3
"""What the nearest-triangle device queries cost (DESIGN.md "Nearest-triangle queries"). On C4 (102,402 triangles,
the default SAH tree, four-wide), for the two point sets of tools/closest_point_probe.py,

* uniform: 1,000,000 points uniform in the scene's box (default_rng(11)),
* surface: the hit points of the 2,073,600 primary rays of the default 1920x1080 view, pushed 0.01 along their
  face normals (coherent, near the surface),

it times, in one run per point set, each as the median of 20 GPU times between two events after 3 warm-ups (with
the fastest and slowest of the 20 as the spread):

* k = 1 of rt_nearest_triangles_device against rt_closest_point_device,
* k = 4, 8 and 16 without a radius and with the radius r_half at which about half the points have a triangle
  inside: the median of the points' closest distances, or, where those pile up at one value (the surface set)
  so that no single radius splits the set, twice a point's own closest distance for every other point and half
  of it for the rest,
* RT_NEAR_COUNT_ALL at k = 1 with r_half (without a radius it counts every triangle: the loop over all of them),
* rt_within_radius_device against rt_closest_point_device, both with r_half.

Every ratio stands next to the spreads of its two sides and says whether they overlap.

The leg "qwork" records, for scene Q of the tests and the 256 in-box points of tests/_closest_point_ref.py with
rmax = 0.05, the evaluations per point of the k = 16 list, the k = 1 list and the verdict for every builder and
width: the numbers tests/test_gpu_nearest.py pins.

Each leg runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/nearest_probe.py out.json [uniform|surface|qwork ...]   (results are merged into out.json)
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
KS = (4, 8, 16)
Q_RMAX = 0.05


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
    path = scenes.write_sphere_grid(QS.SPEC_Q, tempfile.mkdtemp(), "near_q")
    with R.Scene.load(path, device=0) as sc:
        e = sc.export()
        T = np.ascontiguousarray(e["vertices"][e["triangles"].astype(np.int64)], np.float32)
        p = CP.in_box_points(T)
        dp = torch.from_numpy(p).to(dev)
        rm = torch.full((len(p),), Q_RMAX, dtype=torch.float32, device=dev)
        r = dict(triangles=len(T), points=len(p), rmax=Q_RMAX)
        sc.set_profiling(True, count_work=True)

        def counted(fn):
            sc.reset_stats()
            fn()
            torch.cuda.synchronize(dev)
            t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
            return round(t / len(p), 3), round(v / len(p), 3)

        for b in BUILDERS:
            sc.set_builder(b)
            sc.update_vertices(e["vertices"], "rebuild")
            r[b] = {}
            for width in (4, 2):
                sc.tune("bvh_width", width)
                row = {}
                for name, fn in (("k16", lambda: sc.nearest_triangles_device(dp, 16, rmax=rm)),
                                 ("k1", lambda: sc.nearest_triangles_device(dp, 1, rmax=rm)),
                                 ("within", lambda: sc.within_radius_device(dp, rmax=rm)),
                                 ("closest_point", lambda: sc.closest_point_device(dp, rmax=rm))):
                    row[name + "_evaluations_per_point"], row[name + "_node_visits_per_point"] = counted(fn)
                r[b][f"width{width}"] = row
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

    def against(a, b):
        """a over b: the ratio of the medians, both spreads, and whether they overlap."""
        return dict(ratio=round(a["median"] / b["median"], 3), ms=a, against_ms=b,
                    spreads_overlap=bool(a["min"] <= b["max"] and b["min"] <= a["max"]))

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
            del o3, d3, tri, hit, nrm
        else:
            rng = np.random.default_rng(11)
            lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
            pts = torch.from_numpy(rng.uniform(lo, hi, (1_000_000, 3)).astype(np.float32)).to(dev)
        n = len(pts)
        rec1 = torch.empty((n, 4), dtype=torch.int32, device=dev)
        reck = torch.empty((n, max(KS), 4), dtype=torch.int32, device=dev)
        nf = torch.empty((n,), dtype=torch.int32, device=dev)
        wi = torch.empty((n,), dtype=torch.uint8, device=dev)

        _, dist, _ = sc.closest_point_device(pts, out=rec1)
        r_half = float(dist.median().item())
        rm = torch.full((n,), r_half, dtype=torch.float32, device=dev)
        rule = "the median of the closest distances, for every point"
        if not 0.4 <= float((dist < rm).float().mean().item()) <= 0.6:
            # the distances pile up at one value (the surface set: the push distance), so no single radius has
            # about half the points answer: every other point searches twice its closest distance, the rest half
            even = (torch.arange(n, device=dev) % 2 == 0)
            rm = torch.where(torch.isfinite(dist), dist * torch.where(even, 2.0, 0.5), torch.full_like(dist, r_half)).contiguous()
            rule = "per point: twice its closest distance (even index) or half of it (odd index)"

        def out_k(k):
            return (reck.view(-1)[:n * k * 4].view(n, k, 4), nf)

        r = dict(points=n, triangles=int(len(e["triangles"])), r_half=r_half, r_half_rule=rule)
        cp = event_ms(lambda: sc.closest_point_device(pts, out=rec1))
        cp_r = event_ms(lambda: sc.closest_point_device(pts, rmax=rm, out=rec1))
        r["closest_point_ms"], r["closest_point_r_half_ms"] = cp, cp_r
        ref1 = rec1.clone()
        r["answers_inside_r_half"] = int((ref1[:, 0] >= 0).sum().item())

        # k = 1 against the closest-point query
        k1 = event_ms(lambda: sc.nearest_triangles_device(pts, 1, out=out_k(1)))
        k1_r = event_ms(lambda: sc.nearest_triangles_device(pts, 1, rmax=rm, out=out_k(1)))
        r["k1_same_bytes_as_closest_point"] = bool(torch.equal(out_k(1)[0][:, 0], ref1))
        r["k1_over_closest_point"] = against(k1, cp)
        r["k1_r_half_over_closest_point_r_half"] = against(k1_r, cp_r)
        # longer lists, without and with the radius
        for k in KS:
            r[f"k{k}_over_closest_point"] = against(event_ms(lambda: sc.nearest_triangles_device(pts, k, out=out_k(k))), cp)
            r[f"k{k}_r_half_over_closest_point_r_half"] = against(
                event_ms(lambda: sc.nearest_triangles_device(pts, k, rmax=rm, out=out_k(k))), cp_r)
            r[f"k{k}_r_half_mean_rows"] = round(float(nf.float().mean().item()), 3)
        # every candidate inside the radius counted
        call = event_ms(lambda: sc.nearest_triangles_device(pts, 1, rmax=rm, count_all=True, out=out_k(1)))
        r["count_all_k1_r_half_over_k1_r_half"] = against(call, k1_r)
        r["count_all_k1_r_half_over_closest_point_r_half"] = against(call, cp_r)
        r["count_all_mean_count"] = round(float(nf.float().mean().item()), 3)
        # the verdict
        wq = event_ms(lambda: sc.within_radius_device(pts, rmax=rm, out=wi))
        r["within_r_half_over_closest_point_r_half"] = against(wq, cp_r)
        r["within_answers"] = int(wi.sum().item())
        r["within_same_as_closest_point"] = bool(torch.equal(wi != 0, ref1[:, 0] >= 0))
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
        doc = dict(probe="tools/nearest_probe.py", scene="C4 (102,402 triangles), SAH tree, four-wide",
                   runs="median (min, max) of 20 GPU times between events after 3 warm-ups; ratio: of the medians", point_sets={})
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
