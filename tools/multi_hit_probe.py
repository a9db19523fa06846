#!/usr/bin/env python3
"""What the multi-hit device query costs next to the closest-record query and to stepping (DESIGN.md "Multi-hit
device queries"). On C4 (102,402 triangles), for two ray sets,

* primary: the 2,073,600 primary rays of the default 1920x1080 view,
* random:  1,000,000 pairs of standard-normal points x 0.5 (incoherent rays through the scene),

it times, in one run per ray set, each as the median of 20 GPU times between two events after 3 warm-ups (with
the fastest and slowest of the 20 as the spread):

* rt_closest_hit_range_device with NULL bounds (before and after the others: the baseline's own spread),
* rt_multi_hit_range_device at k = 1, 4, 8, 16, and at k = 1 with RT_MULTI_COUNT_ALL,
* stepping for k = 4 and 8: k launches of rt_closest_hit_range_device, each after the first with
  tmin = nextafter(previous distance) (the elementwise step between two launches is part of what is timed).

A second, untimed pass under RT_PROFILE_WORK counts the node visits and triangle tests of each.

Each ray set runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/multi_hit_probe.py out.json [primary|random ...]   (results are merged into out.json)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 240
WARM, N = 3, 20
KS = (1, 4, 8, 16)
PEELS = (4, 8)


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
        if name == "primary":
            p = R.RenderParams(width=wl["width"], height=wl["height"], pf=1, max_lvl=0, lights=[list(x) for x in wl["lights"]])
            rec, _ = sc.trace_frame_samples(p, with_rays=True)
            rec = rec.reshape(-1, 9)
            o, d = np.ascontiguousarray(rec[:, 0:3]), np.ascontiguousarray(rec[:, 3:6])
        else:
            rng = np.random.default_rng(11)
            o = (rng.standard_normal((1_000_000, 3)) * 0.5).astype(np.float32)
            d = (rng.standard_normal((1_000_000, 3)) * 0.5).astype(np.float32)
        n = len(o)
        o3, d3 = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        rec1 = torch.empty((n, 4), dtype=torch.int32, device=dev)
        recs = {k: torch.empty((n, k, 4), dtype=torch.int32, device=dev) for k in KS}
        nh = torch.empty(n, dtype=torch.int32, device=dev)
        inf = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)

        def closest():
            return sc.closest_hit_device(o3, d3, out=rec1)

        def multi(k, count_all=False):
            return lambda: sc.multi_hit_device(o3, d3, k, count_all=count_all, out=(recs[k], nh))

        def peel(k):
            def run():
                tmin = None
                for _ in range(k):
                    _, dist, _ = sc.closest_hit_device(o3, d3, tmin=tmin, out=rec1)
                    tmin = torch.nextafter(dist, inf)
            return run

        r = dict(rays=n)
        closest()
        multi(1)()
        r["k1_equals_closest_record"] = bool(torch.equal(recs[1][:, 0], rec1))
        multi(16, True)()
        total = nh.to(torch.int64)
        r["hits_per_ray_mean"] = round(float(total.sum().item()) / n, 3)
        r["rays_with_more_than_k_hits"] = {str(k): int((total > k).sum().item()) for k in KS}
        r["closest_record_ms"] = event_ms(closest)
        for k in KS:
            r[f"multi_k{k}_ms"] = event_ms(multi(k))
        r["multi_k1_count_all_ms"] = event_ms(multi(1, True))
        for k in PEELS:
            r[f"peel_{k}_launches_ms"] = event_ms(peel(k))
        r["closest_record_ms_again"] = event_ms(closest)
        base = r["closest_record_ms"]["median"]
        for k in KS:
            r[f"ratio_multi_k{k}_over_closest"] = round(r[f"multi_k{k}_ms"]["median"] / base, 3)
        r["ratio_multi_k1_count_all_over_closest"] = round(r["multi_k1_count_all_ms"]["median"] / base, 3)
        for k in PEELS:
            r[f"ratio_peel_{k}_over_multi_k{k}"] = round(r[f"peel_{k}_launches_ms"]["median"] / r[f"multi_k{k}_ms"]["median"], 3)
        calls = [("closest_record", closest)] + [(f"multi_k{k}", multi(k)) for k in KS] + [("multi_k1_count_all", multi(1, True))]
        calls += [(f"peel_{k}_launches", peel(k)) for k in PEELS]
        for key, fn in calls:                                    # untimed: the counting instantiations
            sc.set_profiling(True, count_work=True)
            sc.reset_stats()
            fn()
            torch.cuda.synchronize(dev)
            t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
            sc.set_profiling(False)
            r["work_" + key] = dict(tests_per_ray=round(t / n, 3), visits_per_ray=round(v / n, 3))
    print(name, json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(r, f)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    names = sys.argv[2:] or ["primary", "random"]
    results = {}
    for name in names:                                           # a fresh process per ray set, each under its own limit
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
        doc = dict(probe="tools/multi_hit_probe.py", scene="C4 (102,402 triangles)",
                   runs="median (min, max) of 20 GPU times between events after 3 warm-ups; work: untimed counting pass", ray_sets={})
        if os.path.exists(out_path):
            with open(out_path) as f:
                doc = json.load(f)
        doc["ray_sets"].update(results)
        with open(out_path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
    else:
        main()
