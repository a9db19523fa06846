#!/usr/bin/env python3
"""What the box-overlap device queries cost (DESIGN.md "Box-overlap queries"). On C4 (102,402 triangles), for two
box sets,

* grid: the 2,097,152 cells of a 128^3 grid over the scene's box (a voxeliser's queries, x fastest),
* random: 1,000,000 boxes with centres uniform in the scene's box and edges uniform in [0, 1/32] of its extent per
  axis (default_rng(11)),

it times, in one run per box set, each as the median of 20 GPU times between two events after 3 warm-ups (with the
fastest and slowest of the 20 as the spread), on the trees of the three builders (SAH, LBVH, CLUSTER), four-wide and
binary:

* rt_box_occupied_device (the verdict),
* rt_box_overlap_device at k = 1, 4, 16, and at k = 1 with RT_BOX_COUNT_ALL,
* rt_within_radius_device on the boxes' centres with the half diagonal as the radius (the ball around the box: the
  substitute before this query) and rt_point_inside_device on the centres along +z, the two yardsticks every
  time above is also given as a multiple of,
* the loop over every triangle (RT_ACCEL_BRUTE_FORCE) on the first 4,096 boxes.

A second, untimed pass under RT_PROFILE_WORK counts the leaf triangles met and node visits per box.

Each box set runs in a process of its own under a time limit; the first that fails ends the run.

Usage: python tools/box_overlap_probe.py out.json [grid|random ...]   (results are merged into out.json)
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
GRID = 128
KS = (1, 4, 16)


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
        vlo, vhi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
        if name == "grid":
            edges = [np.linspace(vlo[a], vhi[a], GRID + 1) for a in range(3)]
            iz, iy, ix = np.meshgrid(np.arange(GRID), np.arange(GRID), np.arange(GRID), indexing="ij")
            idx = (ix.ravel(), iy.ravel(), iz.ravel())
            blo = np.stack([edges[a][idx[a]] for a in range(3)], axis=1).astype(np.float32)
            bhi = np.stack([edges[a][idx[a] + 1] for a in range(3)], axis=1).astype(np.float32)
        else:
            rng = np.random.default_rng(11)
            ctr = rng.uniform(vlo, vhi, (1_000_000, 3))
            half = rng.uniform(0, 1 / 64, (1_000_000, 3)) * (vhi - vlo)
            blo, bhi = (ctr - half).astype(np.float32), (ctr + half).astype(np.float32)
        lo, hi = torch.from_numpy(np.ascontiguousarray(blo)).to(dev), torch.from_numpy(np.ascontiguousarray(bhi)).to(dev)
        n = len(lo)
        centre = ((lo + hi) * 0.5).contiguous()
        radius = (0.5 * (hi - lo).norm(dim=1)).contiguous()
        occ = torch.empty((n,), dtype=torch.uint8, device=dev)
        nf = torch.empty((n,), dtype=torch.int32, device=dev)
        lists = {k: torch.empty((n, k), dtype=torch.int32, device=dev) for k in KS}
        within = torch.empty((n,), dtype=torch.uint8, device=dev)
        ins = torch.empty((n,), dtype=torch.uint8, device=dev)
        lob, hib = lo[:N_BRUTE].contiguous(), hi[:N_BRUTE].contiguous()
        occb = torch.empty((N_BRUTE,), dtype=torch.uint8, device=dev)
        nfb = torch.empty((N_BRUTE,), dtype=torch.int32, device=dev)
        listb = torch.empty((N_BRUTE, 16), dtype=torch.int32, device=dev)

        timed = {"occupied": lambda: sc.box_occupied_device(lo, hi, out=occ)}
        for k in KS:
            timed[f"list_k{k}"] = lambda k=k: sc.box_overlap_device(lo, hi, k, out=(lists[k], nf))
        timed["count_all_k1"] = lambda: sc.box_overlap_device(lo, hi, 1, count_all=True, out=(lists[1], nf))
        yard = {"within_radius": lambda: sc.within_radius_device(centre, rmax=radius, out=within),
                "point_inside": lambda: sc.point_inside_device(centre, axis=4, out=ins)}

        r = dict(boxes=n, triangles=int(len(e["triangles"])))
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
                timed["occupied"]()
                got = (lists[16].clone(), nf.clone(), occ.clone())
                if ref is None:
                    ref = got
                    yard["within_radius"]()
                    r["occupied_fraction"] = round(float(occ.float().mean().item()), 4)
                    r["within_radius_fraction"] = round(float(within.float().mean().item()), 4)
                    r["overlaps_per_box_mean"] = round(float(nf.float().mean().item()), 3)
                    r["overlaps_per_box_max"] = int(nf.max().item())
                    r["boxes_with_more_than_16"] = int((nf > 16).sum().item())
                r[key + "_same_bytes_as_first"] = bool(all(torch.equal(a, c) for a, c in zip(got, ref)))
                sc.set_profiling(True, count_work=True)              # untimed: the counting instantiations
                for what in ("occupied", "list_k1", "list_k16", "count_all_k1"):
                    sc.reset_stats()
                    timed[what]()
                    torch.cuda.synchronize(dev)
                    t, v = sc.work_stats(_capi.KERNEL_CLOSEST_HIT)
                    r[f"{key}_{what}_work"] = dict(leaf_triangles_per_box=round(t / n, 3), node_visits_per_box=round(v / n, 3))
                sc.set_profiling(False)
        sc.tune("bvh_width", 4)
        sc.set_accel("brute_force")
        r[f"brute_force_{N_BRUTE}_boxes_occupied_ms"] = event_ms(lambda: sc.box_occupied_device(lob, hib, out=occb))
        r[f"brute_force_{N_BRUTE}_boxes_count_all_k16_ms"] = event_ms(lambda: sc.box_overlap_device(lob, hib, 16, count_all=True, out=(listb, nfb)))
        r["brute_force_same_bytes_as_first"] = bool(torch.equal(listb, ref[0][:N_BRUTE]) and torch.equal(nfb, ref[1][:N_BRUTE])
                                                     and torch.equal(occb, ref[2][:N_BRUTE]))
        r["brute_force_count_all_us_per_box"] = round(r[f"brute_force_{N_BRUTE}_boxes_count_all_k16_ms"]["median"] * 1e3 / N_BRUTE, 3)
        sc.set_accel("bvh")
    print(name, json.dumps(r), flush=True)
    with open(out_path, "w") as f:
        json.dump(r, f)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    names = sys.argv[2:] or ["grid", "random"]
    results = {}
    for name in names:                                           # a fresh process per box set, each under its own limit
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
        doc = dict(probe="tools/box_overlap_probe.py", scene="C4 (102,402 triangles)",
                   runs="median (min, max) of 20 GPU times between events after 3 warm-ups; work: untimed counting pass", box_sets={})
        if os.path.exists(out_path):
            with open(out_path) as f:
                doc = json.load(f)
        doc["box_sets"].update(results)
        with open(out_path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
    else:
        main()
