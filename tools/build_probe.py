#!/usr/bin/env python3
"""What a new tree costs with each builder (DESIGN.md "GPU BVH build"): for C4 and C5 under D(0.01),

* rt_scene_update_vertices(mode="rebuild") with builder "sah" (the host's binned-SAH build and upload),
  with builder "lbvh" (the k_lbvh_* kernels) and with builder "cluster" (the k_cluster_* kernels), from a
  host array and from a device tensor;
* Scene.create with each builder;
* the first mode="auto" update after each kind of build (after the device build the refit tables were
  made by the kernels; after the host build the first refit makes them on the host);
* the frame time, one frame at a time, after each build (same view, same params; the frames must be
  equal bytes), bvh_info and build_info (tree cost, clustering iterations) of every tree; the frame time
  is taken three times per builder, so that the spread of its repeated medians is on record;
* break-even: the frames after which a host SAH rebuild would have paid,
  (T_sah - T_x) / (frame_x - frame_sah) for x = lbvh and cluster, and the frames after which the
  agglomerative build has paid against the Morton one, (T_cluster - T_lbvh) / (frame_lbvh - frame_cluster).

Timing: median of 20 after 3 warm-ups, the host's wall clock around the call (which returns with the
update complete), from an idle device.

Usage: python tools/build_probe.py [out.json] [workload ...]   (default: c4 c5)
profiles/build_probe.json is the two-builder run before RT_BUILD_CLUSTER, profiles/build_probe_cluster.json
the three-builder run.
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
WARM, N = 3, 20
BUILDERS = ("sah", "lbvh", "cluster")


def deform(v, a):
    v = np.array(v, np.float32)
    a = np.float32(a)
    x, y = v[:, 0].copy(), v[:, 1]
    v[:, 0] = x + a * np.sin(np.float32(7) * y + np.float32(1))
    v[:, 2] = v[:, 2] + a * np.cos(np.float32(5) * x)
    return v


def wall_ms(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, warm=WARM, n=N):
    for _ in range(warm):
        fn()
    return round(float(np.median([wall_ms(fn) for _ in range(n)])), 4)


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
        return median_ms(one, warm, n)

    with R.Scene.load(path, device=0) as sc:
        e = sc.export()
    base = e["vertices"]
    two = [deform(base, 0.008), deform(base, 0.01)]   # (alternating, so no call meets the vertices it left)
    dtwo = [torch.from_numpy(v).to(dev) for v in two]
    r = dict(triangles=int(len(e["triangles"])), vertices=int(len(base)))
    frames = {}
    with R.Scene.create(base, e["triangles"], e["tri_mat"], e["materials"], device=0) as sc:
        for builder in BUILDERS:
            sc.set_builder(builder)
            outcomes, k = set(), [0]

            def rebuild(src):
                k[0] += 1
                outcomes.add(sc.update_vertices(src[k[0] & 1], mode="rebuild"))

            r[f"rebuild_{builder}_host_ms"] = median_ms(lambda: rebuild(two))
            r[f"rebuild_{builder}_device_ms"] = median_ms(lambda: rebuild(dtwo))
            r[f"rebuild_{builder}_outcomes"] = sorted(outcomes)
            assert sc.update_vertices(two[0], mode="rebuild").startswith("rebuilt")
            first = []
            r[f"first_refit_after_{builder}_ms"] = round(wall_ms(lambda: first.append(sc.update_vertices(dtwo[1]))), 4)
            r[f"second_refit_after_{builder}_ms"] = round(wall_ms(lambda: first.append(sc.update_vertices(dtwo[0]))), 4)
            assert first == ["refit", "refit"], first
            assert sc.update_vertices(two[1], mode="rebuild").startswith("rebuilt")
            r[f"builder_{builder}"] = list(sc.builder)
            reps = [frame_ms(sc) for _ in range(3)]
            r[f"frame_{builder}_ms"] = float(np.median(reps))
            r[f"frame_{builder}_medians_ms"] = reps
            frames[builder] = buf.cpu().numpy().copy()
            r[f"bvh_info_{builder}"] = sc.bvh_info()
            r[f"build_info_{builder}"] = sc.build_info()
    r["frames_equal"] = bool(all(np.array_equal(frames["sah"], frames[b]) for b in BUILDERS))
    assert r["frames_equal"]
    for builder in BUILDERS:
        def create():
            R.Scene.create(two[1], e["triangles"], e["tri_mat"], e["materials"], device=0, builder=builder).close()
        r[f"create_{builder}_ms"] = median_ms(create, 1, 5)
    r["rebuild_sah_over_lbvh"] = round(r["rebuild_sah_device_ms"] / r["rebuild_lbvh_device_ms"], 1)
    r["frame_lbvh_over_sah"] = round(r["frame_lbvh_ms"] / r["frame_sah_ms"], 3)
    slower = r["frame_lbvh_ms"] - r["frame_sah_ms"]
    r["break_even_frames"] = round((r["rebuild_sah_device_ms"] - r["rebuild_lbvh_device_ms"]) / slower, 1) if slower > 0 else None
    r["frame_cluster_over_sah"] = round(r["frame_cluster_ms"] / r["frame_sah_ms"], 3)
    r["frame_cluster_over_lbvh"] = round(r["frame_cluster_ms"] / r["frame_lbvh_ms"], 3)
    r["frame_median_spread_ms"] = round(max(max(r[f"frame_{b}_medians_ms"]) - min(r[f"frame_{b}_medians_ms"]) for b in BUILDERS), 4)
    slower = r["frame_cluster_ms"] - r["frame_sah_ms"]
    # (read it against frame_median_spread_ms: a frame difference inside that spread gives no break-even)
    r["break_even_frames_cluster_vs_sah"] = round((r["rebuild_sah_device_ms"] - r["rebuild_cluster_device_ms"]) / slower, 1) if slower > 0 else None
    faster = r["frame_lbvh_ms"] - r["frame_cluster_ms"]
    r["break_even_frames_cluster_vs_lbvh"] = round((r["rebuild_cluster_device_ms"] - r["rebuild_lbvh_device_ms"]) / faster, 1) if faster > 0 else None
    r["cluster_pays"] = bool(faster > r["frame_median_spread_ms"])
    results[name] = r
    print(name, json.dumps(r), flush=True)

text = json.dumps(dict(probe="tools/build_probe.py", deformation="D(0.008) and D(0.01) alternating", timing=f"median of {N} after {WARM}, wall clock",
                       workloads=results), indent=1)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
