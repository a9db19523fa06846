#!/usr/bin/env python3
"""What the triangle-distance device queries cost (DESIGN.md "Triangle-distance queries"). On C4 (102,402 triangles),
for the triangle-overlap probe's three query sets,

* displaced: the scene's own triangles translated by a quarter of a sphere radius along (1, 1, 1) / sqrt(3),
* self: the scene's own triangles untranslated with self_index = arange (the clearance of the mesh from itself),
* random: 1,000,000 triangles with centres uniform in the scene's box and vertices within 1/32 of its extent per axis
  of the centre (default_rng(11)),

it times, in one run per query set, each as the median of 20 GPU times between two events after 3 warm-ups (with the
fastest and slowest of the 20 as the spread), on the trees of the three builders (SAH, LBVH, CLUSTER), four-wide and
binary:

* rt_triangle_distance_device (the record, with both point outputs) and rt_triangle_within_device (the verdict),
  each without a radius and with the radius at which half the queries answer (the median of the distances),
* rt_triangle_overlap_device at k = 1 on the same queries and rt_closest_point_device on the queries' centroids, the
  two yardsticks every time above is also given as a multiple of,
* the loop over every triangle (RT_ACCEL_BRUTE_FORCE) on the first 4,096 queries.

A second, untimed pass under RT_PROFILE_WORK counts the triangle evaluations and node visits per query. Every tree's
bytes (records, points, verdicts) are compared with the first tree's, and the first 4,096 with the loop's.

Each query set runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/triangle_distance_probe.py out.json [displaced|self|random ...]   (results are merged into out.json)
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
N_BRUTE = 4096


def one(name, out_path):
    import numpy as np
    import torch

    sys.path.insert(0, HERE)
    import bench
    import raytracert_amd as R
    from raytracert_amd import _capi, scenes

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
        own = verts[np.asarray(e["triangles"], np.int64).reshape(-1, 3)].astype(np.float32)      # [nt, 3, 3]
        vlo, vhi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
        slf = None
        if name == "displaced":
            q = (own.astype(np.float64) + 0.25 * scenes.C4.radius / np.sqrt(3.0)).astype(np.float32)
        elif name == "self":
            q = own
            slf = torch.arange(len(own), dtype=torch.int32, device=dev)
        else:
            rng = np.random.default_rng(11)
            ctr = rng.uniform(vlo, vhi, (1_000_000, 1, 3))
            q = (ctr + rng.uniform(-1 / 32, 1 / 32, (1_000_000, 3, 3)) * (vhi - vlo)).astype(np.float32)
        qt = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        n = len(qt)
        centroids = torch.from_numpy(np.ascontiguousarray(q.astype(np.float64).mean(axis=1).astype(np.float32))).to(dev)
        rec = torch.empty((n, 4), dtype=torch.int32, device=dev)
        qp, pp = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
        within = torch.empty((n,), dtype=torch.uint8, device=dev)
        olist, onf = torch.empty((n, 1), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        prec = torch.empty((n, 4), dtype=torch.int32, device=dev)
        qb = qt[:N_BRUTE].contiguous()
        slfb = None if slf is None else slf[:N_BRUTE].contiguous()
        recb = torch.empty((N_BRUTE, 4), dtype=torch.int32, device=dev)
        qpb, ppb = torch.empty((N_BRUTE, 3), dtype=torch.float32, device=dev), torch.empty((N_BRUTE, 3), dtype=torch.float32, device=dev)
        withinb = torch.empty((N_BRUTE,), dtype=torch.uint8, device=dev)

        # the radius at which half the queries answer: the median of the distances
        sc.triangle_distance(qt, self_index=slf, out=rec)
        dist = rec[:, 1].view(torch.float32)
        half = float(dist[torch.isfinite(dist)].median().item())
        half = half if half > 0 else float(dist[dist > 0].min().item())      # (more than half the queries overlap: the smallest clearance)
        rmax = torch.full((n,), half, dtype=torch.float32, device=dev)
        rmaxb = rmax[:N_BRUTE].contiguous()

        timed = {"record": lambda: sc.triangle_distance(qt, self_index=slf, want_points=True, out=(rec, qp, pp)),
                 "record_radius": lambda: sc.triangle_distance(qt, rmax=rmax, self_index=slf, want_points=True, out=(rec, qp, pp)),
                 "within": lambda: sc.triangle_within(qt, self_index=slf, out=within),
                 "within_radius": lambda: sc.triangle_within(qt, rmax=rmax, self_index=slf, out=within)}
        yard = {"overlap_k1": lambda: sc.triangle_overlap_device(qt, 1, self_index=slf, out=(olist, onf)),
                "closest_point": lambda: sc.closest_point_device(centroids, out=prec)}

        r = dict(queries=n, triangles=int(len(own)), radius=round(half, 6))
        ref = None
        for b in BUILDERS:
            sc.set_builder(b)
            sc.update_vertices(verts, "rebuild")
            for width in (4, 2):
                sc.tune("bvh_width", width)
                key = f"{b}_width{width}"
                for what, fn in yard.items():
                    r[f"{key}_{what}_ms"] = event_ms(fn)
                for what, fn in timed.items():
                    t = r[f"{key}_{what}_ms"] = event_ms(fn)
                    for y in yard:
                        r[f"{key}_{what}_over_{y}"] = round(t["median"] / r[f"{key}_{y}_ms"]["median"], 3)
                got = []
                for what in ("record", "record_radius"):
                    timed[what]()
                    got += [rec.clone(), qp.clone(), pp.clone()]
                timed["within_radius"]()
                got.append(within.clone())
                if ref is None:
                    ref = got
                    d = got[0][:, 1].view(torch.float32)
                    r["distance_zero_fraction"] = round(float((d == 0).float().mean().item()), 4)
                    r["distance_median"] = round(float(d[torch.isfinite(d)].median().item()), 6)
                    r["answers_within_radius_fraction"] = round(float(within.float().mean().item()), 4)
                r[key + "_same_bytes_as_first"] = bool(all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                         c.view(torch.int32) if c.dtype == torch.float32 else c)
                                                           for a, c in zip(got, ref)))
                sc.set_profiling(True, count_work=True)              # untimed: the counting instantiations
                for what in timed:
                    sc.reset_stats()
                    timed[what]()
                    torch.cuda.synchronize(dev)
                    t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                    r[f"{key}_{what}_work"] = dict(evaluations_per_query=round(t / n, 3), node_visits_per_query=round(v / n, 3))
                sc.set_profiling(False)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        r[f"brute_force_{N_BRUTE}_queries_record_ms"] = event_ms(lambda: sc.triangle_distance(qb, self_index=slfb, want_points=True,
                                                                                              out=(recb, qpb, ppb)))
        same = torch.equal(recb, ref[0][:N_BRUTE]) and torch.equal(qpb.view(torch.int32), ref[1][:N_BRUTE].view(torch.int32)) \
            and torch.equal(ppb.view(torch.int32), ref[2][:N_BRUTE].view(torch.int32))
        r[f"brute_force_{N_BRUTE}_queries_within_radius_ms"] = event_ms(lambda: sc.triangle_within(qb, rmax=rmaxb, self_index=slfb, out=withinb))
        r["brute_force_same_bytes_as_first"] = bool(same and torch.equal(withinb, ref[6][:N_BRUTE]))
        r["brute_force_record_us_per_query"] = round(r[f"brute_force_{N_BRUTE}_queries_record_ms"]["median"] * 1e3 / N_BRUTE, 3)
        sc.set_accel("bvh")
    print(name, json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(r, f)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    names = sys.argv[2:] or ["displaced", "self", "random"]
    results = {}
    for name in names:                                           # a fresh process per query set, each under its own limit
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
        doc = dict(probe="tools/triangle_distance_probe.py", scene="C4 (102,402 triangles)",
                   runs="median (min, max) of 20 GPU times between events after 3 warm-ups; work: untimed counting pass", query_sets={})
        if os.path.exists(out_path):
            with open(out_path) as f:
                doc = json.load(f)
        doc["query_sets"].update(results)
        with open(out_path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
    else:
        main()
