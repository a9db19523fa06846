#!/usr/bin/env python3
"""Host time of one small device-resident query call (n = 64 on the 512-triangle blob of tests/_inside_ref.py), one
entry per family: what the argument rules and the launch frame of rt_capi.cpp, and the checks of the Scene methods,
cost per call, which the kernels' time hides at any larger n. Builds are compared inside ONE process: each build is
a library with a Python package (its wrapper), all are loaded side by side, and they take turns in blocks of calls,
the order reversed every round, so that what differs between two processes (placement, clocks: about 1 us on a
5 us call, more than any build differs by) is common to them. Per entry and build: the median host time of each
block, for the C entry alone (arguments built beforehand) and for the Scene method (out tensors given), with the
GPU busy behind earlier calls (no synchronisation inside a timed call; one every 256 calls, not timed).

Usage: python tools/query_call_probe.py [--calls N] [--rounds R] [--json out.json] [NAME=LIB[@PACKAGE_ROOT] ...]
The first build is the reference: the table says where every other build's median over its blocks lies against
the range of the reference's block medians (inside, below: faster than its fastest block, or ABOVE). Without
builds: the tree's own. PACKAGE_ROOT holds a raytracert_amd/ and its include/ (default: this tree), e.g. a
`git archive` of another commit.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=2000, help="calls per block")
ap.add_argument("--rounds", type=int, default=12, help="blocks per build, entry and kind")
ap.add_argument("--json", default=None)
ap.add_argument("builds", nargs="*", default=["tree=" + os.path.join(HERE, "raytracert_amd", "librtamd.so")])
args = ap.parse_args()
sys.path.insert(0, os.path.join(HERE, "tests"))
import _inside_ref as IR  # noqa: E402

dev = torch.device("cuda", 0)
N, K = 64, 4
V, tri = IR.blob()


def load(spec):
    """One build: its package imported under the usual name (then taken out of sys.modules again, so the next
    build imports its own), bound to its library."""
    name, rest = spec.split("=", 1)
    path, _, root = rest.partition("@")
    os.environ["RTAMD_LIB"] = os.path.abspath(path)
    for m in [m for m in sys.modules if m == "raytracert_amd" or m.startswith("raytracert_amd.")]:
        del sys.modules[m]
    sys.path.insert(0, os.path.abspath(root or HERE))
    import raytracert_amd as R
    from raytracert_amd import _capi
    sys.path.pop(0)
    assert _capi.LIB_PATH == os.environ["RTAMD_LIB"] and os.path.dirname(os.path.dirname(R.__file__)) == os.path.abspath(root or HERE)
    sc = R.Scene.create(np.ascontiguousarray(V, np.float32), tri, np.zeros(len(tri), np.uint32), IR.MATERIALS, device=0)
    return dict(name=name, capi=_capi, lib=_capi.lib(), sc=sc)


rng = np.random.default_rng(3)
p = torch.from_numpy(rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)).to(dev)
o = torch.from_numpy(np.concatenate([rng.uniform(-1.3, 1.3, (N, 2)), np.full((N, 1), 4.0)], axis=1).astype(np.float32)).to(dev)
d = o - torch.tensor([0.0, 0.0, 8.0], device=dev)      # (along -z through the blob's box)
lo, hi = p - 0.1, p + 0.1
qt = torch.stack([p, p + torch.tensor([0.2, 0.0, 0.05], device=dev), p + torch.tensor([0.0, 0.2, -0.05], device=dev)], dim=1).contiguous()
rec = torch.zeros((N, 4), dtype=torch.int32, device=dev)
reck = torch.zeros((N, K, 4), dtype=torch.int32, device=dev)
idx = torch.zeros(N, dtype=torch.int32, device=dev)
idk = torch.zeros((N, K), dtype=torch.int32, device=dev)
pts = torch.zeros((N, 3), dtype=torch.float32, device=dev)
P = {k: C.c_void_p(t.data_ptr()) for k, t in dict(o=o, d=d, p=p, lo=lo, hi=hi, qt=qt, rec=rec, reck=reck, idx=idx, idk=idk, pts=pts).items()}


def entries(b):
    """Per family (C entry, Scene method) of build b."""
    lib, h, sc, cap = b["lib"], b["sc"]._h, b["sc"], b["capi"]
    return {
        "rays: rt_intersect_mesh_device": (
            lambda: lib.rt_intersect_mesh_device(h, P["o"], P["d"], 3, N, None, P["idx"], P["pts"], None),
            lambda: sc.intersect_mesh_device(o, d, out=(idx, pts))),
        "ranged rays: rt_closest_hit_range_device": (
            lambda: lib.rt_closest_hit_range_device(h, P["o"], P["d"], 3, N, None, None, None, cap.RANGE_TO_DEST, P["rec"], None, None),
            lambda: sc.closest_hit_device(o, d, to_dest=True, out=rec)),
        "ray lists: rt_multi_hit_range_device": (
            lambda: lib.rt_multi_hit_range_device(h, P["o"], P["d"], 3, N, None, None, None, 0, K, P["reck"], P["idx"], None),
            lambda: sc.multi_hit_device(o, d, K, out=(reck, idx))),
        "points: rt_closest_point_device": (
            lambda: lib.rt_closest_point_device(h, P["p"], 3, N, None, None, 0, P["rec"], None, None),
            lambda: sc.closest_point_device(p, out=rec)),
        "point lists: rt_nearest_triangles_device": (
            lambda: lib.rt_nearest_triangles_device(h, P["p"], 3, N, None, None, 0, K, P["reck"], P["idx"], None, None),
            lambda: sc.nearest_triangles_device(p, K, out=(reck, idx))),
        "inside (two launches): rt_signed_distance_device": (
            lambda: lib.rt_signed_distance_device(h, P["p"], 3, N, None, None, cap.AXIS_POS_Z, 0, P["rec"], None, P["idx"], None),
            lambda: sc.signed_distance_device(p, out=rec)),
        "boxes: rt_box_overlap_device": (
            lambda: lib.rt_box_overlap_device(h, P["lo"], P["hi"], 3, N, None, None, 0, K, P["idk"], P["idx"], None),
            lambda: sc.box_overlap_device(lo, hi, K, out=(idk, idx))),
        "triangles: rt_triangle_overlap_device": (
            lambda: lib.rt_triangle_overlap_device(h, P["qt"], 3, N, None, None, None, 0, K, P["idk"], P["idx"], None),
            lambda: sc.triangle_overlap_device(qt, K, out=(idk, idx))),
    }


def block_us(fn, calls):
    t = []
    for i in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
        if i % 256 == 255:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    return round(float(np.median(t)) * 1e6, 3)


builds = [load(s) for s in args.builds]
assert len({b["lib"]._handle for b in builds}) == len(builds), "two builds name one library file"
E = [entries(b) for b in builds]
doc = dict(probe="tools/query_call_probe.py", n=N, calls_per_block=args.calls, rounds=args.rounds,
           builds={b["name"]: dict(library=b["capi"].LIB_PATH, wrapper=os.path.dirname(b["capi"].__file__)) for b in builds}, block_medians_us={})
print(f"# {' '.join(sys.argv[1:])}")
print(f"# host time per call [us], n = {N}: median over {args.rounds} blocks of {args.calls} calls of each block's median (fastest-slowest block);")
print(f"# against {builds[0]['name']}: the build's median against the range of {builds[0]['name']}'s block medians (in brackets: how many of its blocks lie inside)")
print(f"{'entry':60s} " + " ".join(f"{b['name']:26s}" for b in builds) + f" against {builds[0]['name']}")
for name in E[0]:
    for kind, label in ((0, "c entry"), (1, "method")):
        for e in E:
            assert kind or e[name][0]() == 0, name
            block_us(e[name][kind], 512)
        rows = [[] for _ in builds]
        for r in range(args.rounds):
            for i in (range(len(builds)) if r % 2 == 0 else reversed(range(len(builds)))):
                rows[i].append(block_us(E[i][name][kind], args.calls))
        doc["block_medians_us"][f"{label}, {name}"] = {b["name"]: rows[i] for i, b in enumerate(builds)}
        lo_ref, hi_ref = min(rows[0]), max(rows[0])
        verdict = ", ".join(f"{'below' if statistics.median(r) < lo_ref else 'ABOVE' if statistics.median(r) > hi_ref else 'inside'} "
                            f"({sum(lo_ref <= x <= hi_ref for x in r)} of {len(r)})" for r in rows[1:])
        print(f"{label + ', ' + name:60s} " + " ".join(f"{statistics.median(r):7.3f} ({min(r):.3f}-{max(r):.3f})".ljust(26) for r in rows) + " " + verdict)
if args.json:
    with open(args.json, "w") as f:
        f.write(json.dumps(doc) + "\n")
