#!/usr/bin/env python3
"""What a change of topology costs (DESIGN.md "Topology changes"): for C4 and C5, two meshes alternating,
M0 = the workload's mesh under D(0.008) and M1 = under D(0.01) with the last 10% of the triangles dropped (so
the counts change both ways every call),

(a) rt_scene_set_mesh_device from device tensors, builders "lbvh" and "cluster";
(b) rt_scene_set_mesh from host arrays, the same builders;
(c) rt_scene_destroy + rt_scene_create_ex from host arrays, the only route before rt_scene_set_mesh,
    builders "lbvh", "cluster" and "sah";

and in the same run, per builder, the RT_UPDATE_REBUILD time from a device tensor (the floor: the same
kernels without validation, copies of indices and materials, or state reset), and the one-at-a-time frame
time of the scene after (a) against a fresh scene of the same mesh (medians of 50 frames after 40: three for
the scene after (a), five for the fresh scene, whose repeated medians' spread and whose individual frames'
fastest-slowest range are both on record; the frames must be equal bytes).

Timing: median of 20 after 3 warm-ups, the host's wall clock around the call (which returns with the
replacement complete), from an idle device.

Usage: python tools/set_mesh_probe.py [out.json] [workload ...]   (default: c4 c5)
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
GPU_BUILDERS = ("lbvh", "cluster")


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

    def frame_samples(sc, warm=40, n=50):
        """n one-at-a-time frame times (ms) after `warm` frames."""
        def one():
            sc.render_frame_device(p, 16, 16, buf.data_ptr(), buf.numel(), st.cuda_stream)
            torch.cuda.synchronize(dev)
        for _ in range(warm):
            one()
        return [wall_ms(one) for _ in range(n)]

    with R.Scene.load(path, device=0) as sc:
        e = sc.export()
    base, tris, tmat, mats = e["vertices"], e["triangles"], e["tri_mat"], e["materials"]
    keep = len(tris) - len(tris) // 10
    meshes = [(deform(base, 0.008), tris, tmat), (deform(base, 0.01), np.ascontiguousarray(tris[:keep]), np.ascontiguousarray(tmat[:keep]))]
    dmeshes = [(torch.from_numpy(v).to(dev), torch.from_numpy(t.view(np.int32)).to(dev), torch.from_numpy(m.view(np.int32)).to(dev))
               for v, t, m in meshes]
    dverts = [torch.from_numpy(deform(base, a)).to(dev) for a in (0.008, 0.01)]
    r = dict(vertices=int(len(base)), triangles=[int(len(m[1])) for m in meshes])
    for builder in GPU_BUILDERS:
        with R.Scene.create(*meshes[0], mats, device=0, builder=builder) as sc:
            outcomes, k = set(), [0]

            def set_mesh(src):
                k[0] += 1
                outcomes.add(sc.set_mesh(*src[k[0] & 1]))

            def rebuild():
                k[0] += 1
                outcomes.add(sc.update_vertices(dverts[k[0] & 1], mode="rebuild"))

            r[f"rebuild_floor_{builder}_ms"] = median_ms(rebuild)
            r[f"set_mesh_device_{builder}_ms"] = median_ms(lambda: set_mesh(dmeshes))
            r[f"set_mesh_host_{builder}_ms"] = median_ms(lambda: set_mesh(meshes))
            r[f"outcomes_{builder}"] = sorted(outcomes)
            assert outcomes == {"rebuilt_" + builder}, outcomes
            # the frame after (a), on M0, against a fresh scene of M0
            sc.set_mesh(*dmeshes[1])
            sc.set_mesh(*dmeshes[0])
            assert sc.counts()[:2] == (len(base), len(tris))
            after_reps = [frame_samples(sc) for _ in range(3)]
            r[f"frame_after_set_mesh_{builder}_medians_ms"] = [round(float(np.median(x)), 4) for x in after_reps]
            r[f"frame_after_set_mesh_{builder}_ms"] = float(np.median(r[f"frame_after_set_mesh_{builder}_medians_ms"]))
            after = buf.cpu().numpy().copy()
        with R.Scene.create(*meshes[0], mats, device=0, builder=builder) as fresh:
            fresh_reps = [frame_samples(fresh) for _ in range(5)]
            reps = [round(float(np.median(x)), 4) for x in fresh_reps]
            r[f"frame_fresh_{builder}_medians_ms"] = reps
            r[f"frame_fresh_{builder}_fastest_slowest_ms"] = [round(min(min(x) for x in fresh_reps), 4), round(max(max(x) for x in fresh_reps), 4)]
            r[f"frame_fresh_{builder}_ms"] = float(np.median(reps))
            r[f"frames_equal_{builder}"] = bool(np.array_equal(after, buf.cpu().numpy()))
            assert r[f"frames_equal_{builder}"]
        spread = max(reps) - min(reps)
        r[f"frame_fresh_{builder}_spread_ms"] = round(spread, 4)
        # two readings of "within the fresh scene's spread": the spread of its five repeated medians around
        # their median (tight: a few microseconds), and the fastest-slowest range of its individual frames
        r[f"frame_after_within_spread_{builder}"] = bool(abs(r[f"frame_after_set_mesh_{builder}_ms"] - r[f"frame_fresh_{builder}_ms"]) <= spread)
        lo, hi = r[f"frame_fresh_{builder}_fastest_slowest_ms"]
        r[f"frame_after_within_fastest_slowest_{builder}"] = bool(lo <= r[f"frame_after_set_mesh_{builder}_ms"] <= hi)
    for builder in GPU_BUILDERS + ("sah",):
        holder, k = [R.Scene.create(*meshes[0], mats, device=0, builder=builder)], [0]

        def recreate():
            k[0] += 1
            holder[0].close()
            holder[0] = R.Scene.create(*meshes[k[0] & 1], mats, device=0, builder=builder)

        r[f"recreate_{builder}_ms"] = median_ms(recreate, 2, 10 if builder == "sah" else N)
        holder[0].close()
    for builder in GPU_BUILDERS:
        a = r[f"set_mesh_device_{builder}_ms"]
        r[f"recreate_over_set_mesh_device_{builder}"] = round(r[f"recreate_{builder}_ms"] / a, 2)
        r[f"recreate_sah_over_set_mesh_device_{builder}"] = round(r["recreate_sah_ms"] / a, 2)
        r[f"set_mesh_device_minus_floor_{builder}_ms"] = round(a - r[f"rebuild_floor_{builder}_ms"], 4)
        r[f"set_mesh_below_recreate_{builder}"] = bool(a < r[f"recreate_{builder}_ms"])
    results[name] = r
    print(name, json.dumps(r), flush=True)

text = json.dumps(dict(probe="tools/set_mesh_probe.py", meshes="M0 = D(0.008); M1 = D(0.01) without the last 10% of the triangles; alternating",
                       timing=f"median of {N} after {WARM} (re-creation with the SAH builder: 10 after 2), wall clock", workloads=results), indent=1)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
