#!/usr/bin/env python3
"""What the triangle-overlap device queries cost (DESIGN.md "Triangle-overlap queries"). On C4 (102,402 triangles),
for three query sets,

* displaced: the scene's own triangles translated by a quarter of a sphere radius along (1, 1, 1) / sqrt(3) (mesh
  against displaced mesh),
* self: the scene's own triangles untranslated with self_index = after = arange (self-intersection),
* random: 1,000,000 triangles with centres uniform in the scene's box and vertices within 1/32 of its extent per axis
  of the centre (default_rng(11)),

it times, in one run per query set, each as the median of 20 GPU times between two events after 3 warm-ups (with the
fastest and slowest of the 20 as the spread), on the trees of the three builders (SAH, LBVH, CLUSTER), four-wide and
binary:

* rt_triangle_collides_device (the verdict),
* rt_triangle_overlap_device at k = 1, 4, 16, and at k = 1 with RT_TRI_COUNT_ALL,
* rt_box_occupied_device and rt_box_overlap_device (k = 16) on the query triangles' bounding boxes, the two yardsticks
  every time above is also given as a multiple of,
* the loop over every triangle (RT_ACCEL_BRUTE_FORCE) on the first 4,096 queries.

A second, untimed pass under RT_PROFILE_WORK counts the leaf triangles met and node visits per query. Every tree's
bytes (the k = 16 list, the counts and the verdicts) are compared with the first tree's, and the first 4,096 with the
loop's.

Each query set runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/triangle_overlap_probe.py out.json [displaced|self|random ...]   (results are merged into out.json)
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
KS = (1, 4, 16)


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
        slf = aft = None
        if name == "displaced":
            q = (own.astype(np.float64) + 0.25 * scenes.C4.radius / np.sqrt(3.0)).astype(np.float32)
        elif name == "self":
            q = own
            slf = aft = torch.arange(len(own), dtype=torch.int32, device=dev)
        else:
            rng = np.random.default_rng(11)
            ctr = rng.uniform(vlo, vhi, (1_000_000, 1, 3))
            q = (ctr + rng.uniform(-1 / 32, 1 / 32, (1_000_000, 3, 3)) * (vhi - vlo)).astype(np.float32)
        qt = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        n = len(qt)
        lo, hi = qt.min(dim=1).values.contiguous(), qt.max(dim=1).values.contiguous()
        col = torch.empty((n,), dtype=torch.uint8, device=dev)
        nf = torch.empty((n,), dtype=torch.int32, device=dev)
        lists = {k: torch.empty((n, k), dtype=torch.int32, device=dev) for k in KS}
        occ = torch.empty((n,), dtype=torch.uint8, device=dev)
        bnf = torch.empty((n,), dtype=torch.int32, device=dev)
        blist = torch.empty((n, 16), dtype=torch.int32, device=dev)
        qb = qt[:N_BRUTE].contiguous()
        slfb = None if slf is None else slf[:N_BRUTE].contiguous()
        colb = torch.empty((N_BRUTE,), dtype=torch.uint8, device=dev)
        nfb = torch.empty((N_BRUTE,), dtype=torch.int32, device=dev)
        listb = torch.empty((N_BRUTE, 16), dtype=torch.int32, device=dev)

        timed = {"collides": lambda: sc.triangle_collides_device(qt, self_index=slf, out=col)}
        for k in KS:
            timed[f"list_k{k}"] = lambda k=k: sc.triangle_overlap_device(qt, k, after=aft, self_index=slf, out=(lists[k], nf))
        timed["count_all_k1"] = lambda: sc.triangle_overlap_device(qt, 1, after=aft, self_index=slf, count_all=True, out=(lists[1], nf))
        yard = {"box_occupied": lambda: sc.box_occupied_device(lo, hi, out=occ),
                "box_list_k16": lambda: sc.box_overlap_device(lo, hi, 16, after=aft, out=(blist, bnf))}

        r = dict(queries=n, triangles=int(len(own)))
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
                timed["list_k16"]()
                timed["count_all_k1"]()
                timed["collides"]()
                got = (lists[16].clone(), nf.clone(), col.clone())
                if ref is None:
                    ref = got
                    yard["box_occupied"]()
                    sc.box_overlap_device(lo, hi, 1, after=aft, count_all=True, out=(lists[1], bnf))
                    r["collides_fraction"] = round(float(col.float().mean().item()), 4)
                    r["box_occupied_fraction"] = round(float(occ.float().mean().item()), 4)
                    r["overlaps_per_query_mean"] = round(float(nf.float().mean().item()), 3)
                    r["overlaps_per_query_max"] = int(nf.max().item())
                    r["queries_with_more_than_16"] = int((nf > 16).sum().item())
                    r["box_overlaps_per_query_mean"] = round(float(bnf.float().mean().item()), 3)
                r[key + "_same_bytes_as_first"] = bool(all(torch.equal(a, c) for a, c in zip(got, ref)))
                sc.set_profiling(True, count_work=True)              # untimed: the counting instantiations
                for what in ("collides", "list_k1", "list_k16", "count_all_k1"):
                    sc.reset_stats()
                    timed[what]()
                    torch.cuda.synchronize(dev)
                    t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                    r[f"{key}_{what}_work"] = dict(leaf_triangles_per_query=round(t / n, 3), node_visits_per_query=round(v / n, 3))
                sc.set_profiling(False)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        aftb = None if aft is None else aft[:N_BRUTE].contiguous()
        r[f"brute_force_{N_BRUTE}_queries_collides_ms"] = event_ms(lambda: sc.triangle_collides_device(qb, self_index=slfb, out=colb))
        r[f"brute_force_{N_BRUTE}_queries_count_all_k16_ms"] = event_ms(
            lambda: sc.triangle_overlap_device(qb, 16, after=aftb, self_index=slfb, count_all=True, out=(listb, nfb)))
        r["brute_force_same_bytes_as_first"] = bool(torch.equal(listb, ref[0][:N_BRUTE]) and torch.equal(nfb, ref[1][:N_BRUTE])
                                                     and torch.equal(colb, ref[2][:N_BRUTE]))
        r["brute_force_count_all_us_per_query"] = round(r[f"brute_force_{N_BRUTE}_queries_count_all_k16_ms"]["median"] * 1e3 / N_BRUTE, 3)
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
        doc = dict(probe="tools/triangle_overlap_probe.py", scene="C4 (102,402 triangles)",
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
