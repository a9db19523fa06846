"""Every device-resident query entry goes through the one launch frame of rt_capi.cpp (run_query): it runs on the
caller's stream, and a query queued after update_vertices answers for the new vertices. Per entry, on the closed
blob of tests/_inside_ref.py with 65 queries (one full wave and one lane): the query on stream A, the same on
stream B, a refit, the query on A again; the first two are, byte for byte, the call made on the default stream
before the update, the third the call made there after it. This pins the stream and the update for each entry;
it is no race detector (a missing wait could still pass)."""
import numpy as np
import pytest
import torch

import raytracert_amd as R

import _inside_ref as IR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
N = 65
K = 4
GROW = F32(1.25)        # the update: the blob scaled about its centre (a refit; every answer below changes)


def _queries():
    """65 directions on a spiral over the sphere with radii 0.3 .. 1.9: the blob's surface lies at 0.72 .. 1.28 of
    its centre before the update and at 0.9 .. 1.6 after it, so points, boxes and triangles at several radii change
    sides, and of the rays along -z at these offsets from the axis several miss before and hit after."""
    i = np.arange(N, dtype=np.float64)
    z = 1.0 - 2.0 * (i + 0.5) / N
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    d = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], axis=1)
    p = (d * (0.3 + 1.6 * i / (N - 1))[:, None]).astype(F32)
    rho = (0.3 + 1.6 * i / (N - 1))
    xy = np.stack([rho * np.cos(phi), rho * np.sin(phi)], axis=1)
    o = np.concatenate([xy, np.full((N, 1), 4.0)], axis=1).astype(F32)
    e = np.concatenate([xy, np.full((N, 1), -4.0)], axis=1).astype(F32)
    tri = np.stack([p, p + np.array([0.2, 0.0, 0.05], F32), p + np.array([0.0, 0.2, -0.05], F32)], axis=1).astype(F32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(o=dev(o), d=dev(e), p=dev(p), lo=dev(p - F32(0.1)), hi=dev(p + F32(0.1)), tri=dev(tri),
                rmax=torch.full((N,), 0.15, dtype=torch.float32, device=DEV))


# the entries, by their Scene method: (name, call(scene, queries, stream))
ENTRIES = [
    ("intersect_mesh_device", lambda sc, q, st: sc.intersect_mesh_device(q["o"], q["d"], stream=st)),
    ("occluded_device", lambda sc, q, st: sc.occluded_device(q["o"], q["d"], stream=st)),
    ("closest_hit_device", lambda sc, q, st: sc.closest_hit_device(q["o"], q["d"], to_dest=True, want_points=True, stream=st)),
    ("occluded_range_device", lambda sc, q, st: sc.occluded_range_device(q["o"], q["d"], to_dest=True, stream=st)),
    ("multi_hit_device", lambda sc, q, st: sc.multi_hit_device(q["o"], q["d"], K, count_all=True, stream=st)),
    ("closest_point_device", lambda sc, q, st: sc.closest_point_device(q["p"], want_points=True, stream=st)),
    ("nearest_triangles_device", lambda sc, q, st: sc.nearest_triangles_device(q["p"], K, count_all=True, want_points=True, stream=st)),
    ("within_radius_device", lambda sc, q, st: sc.within_radius_device(q["p"], rmax=q["rmax"], stream=st)),
    ("point_inside_device", lambda sc, q, st: sc.point_inside_device(q["p"], crossings=True, stream=st)),
    ("signed_distance_device", lambda sc, q, st: sc.signed_distance_device(q["p"], want_points=True, stream=st)),
    ("box_overlap_device", lambda sc, q, st: sc.box_overlap_device(q["lo"], q["hi"], K, count_all=True, stream=st)),
    ("box_occupied_device", lambda sc, q, st: sc.box_occupied_device(q["lo"], q["hi"], stream=st)),
    ("triangle_overlap_device", lambda sc, q, st: sc.triangle_overlap_device(q["tri"], K, count_all=True, stream=st)),
    ("triangle_collides_device", lambda sc, q, st: sc.triangle_collides_device(q["tri"], stream=st)),
]


@pytest.fixture(scope="module")
def frame(gpu_available):
    V, tri = IR.blob()
    V = np.ascontiguousarray(V, F32)
    with R.Scene.create(V, tri, np.zeros(len(tri), np.uint32), IR.MATERIALS, device=0) as sc:
        q = _queries()
        torch.cuda.synchronize(DEV)       # the queries are made; the side streams only read them
        yield dict(sc=sc, q=q, V0=V, V1=(V * GROW).astype(F32), A=torch.cuda.Stream(device=DEV), B=torch.cuda.Stream(device=DEV))


def _bytes(res):
    return tuple(t.cpu().numpy().tobytes() for t in (res if isinstance(res, tuple) else (res,)))


def test_every_entry_is_listed():
    """The list above against the Scene's methods (the renderers and the traced colour use a workspace and a
    pipeline, not the frame): a new *_device query method has to be added to it."""
    have = {m for m in dir(R.Scene) if m.endswith("_device") and not m.startswith(("render_", "perform_"))}
    assert have == {name for name, _ in ENTRIES}


@pytest.mark.parametrize("name,call", ENTRIES, ids=[name for name, _ in ENTRIES])
def test_entry_runs_on_the_callers_stream_and_sees_the_update(frame, name, call):
    sc, q, A, B = frame["sc"], frame["q"], frame["A"], frame["B"]
    assert sc.update_vertices(frame["V0"]) == "refit"
    before = _bytes(call(sc, q, None))                  # (the default stream; .cpu() waits for it)
    with torch.cuda.stream(A):                          # (current too: the result tensors are made and filled on it)
        on_a = call(sc, q, A)
    with torch.cuda.stream(B):
        on_b = call(sc, q, B)
    assert sc.update_vertices(frame["V1"]) == "refit"
    with torch.cuda.stream(A):
        on_a_after = call(sc, q, A)
    A.synchronize()
    B.synchronize()
    after = _bytes(call(sc, q, None))
    assert before != after, f"{name}: the update changes no answer, so the test would pass without it"
    assert _bytes(on_a) == before, f"{name}: stream A before the update"
    assert _bytes(on_b) == before, f"{name}: stream B before the update"
    assert _bytes(on_a_after) == after, f"{name}: stream A after the update"
