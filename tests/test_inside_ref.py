"""The restatement of the inside queries (tests/_inside_ref.py, what tests/test_gpu_inside.py compares the GPU's
bytes with) against things that do not share its arithmetic, on the CPU:

- an independent float64 winding number (summed solid angles) on the blob and the nested blob, for uniform points
  and for points placed exactly under vertices, along +z, -x and +y: every point whose winding number is within
  0.01 of an integer (every point not within rounding of the surface) has that integer's parity;
- the cube with the 125 grid points, all six directions: strictly interior points are inside, points with a
  coordinate outside [0, 2] are outside. Many of these points lie exactly under shared edges and vertices;
- the reason for the query: for the cube's interior points under a face diagonal, the parity of a plain
  per-triangle hit count (tests/_multi_hit_ref.py's count of all accepted triangles along the same direction) is
  wrong, because both triangles at the diagonal accept the ray;
- room for the GPU test's culling cap: the mean number of triangles whose acceptance-box column holds the point is
  far below the triangle count.
"""
import numpy as np
import pytest

from raytracert_amd.api import bvh_acceptance_box

import _inside_ref as IR
import _multi_hit_ref as MH
import _range_ref as RR

F32 = np.float32
DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)


@pytest.mark.parametrize("mesh", ["blob", "nested"])
@pytest.mark.parametrize("axis", [4, 1, 2])
def test_parity_is_the_winding_numbers(mesh, axis):
    V, tri = IR.MESHES[mesh]()
    k = axis >> 1
    p = np.concatenate([IR.uniform_points(V, 600, 11 + axis), IR.under_vertex_points(V, k, 100, 21 + axis)])
    w = IR.winding_number(p, V, tri)
    clear = np.abs(w - np.rint(w)) < 0.01
    assert clear.sum() >= len(p) - 5, f"{(~clear).sum()} points within rounding of the surface"
    cr = IR.crossings(p, V, tri, axis)
    got, want = IR.inside(cr), (np.rint(w).astype(np.int64) & 1).astype(np.uint8)
    bad = np.flatnonzero(clear & (got != want))
    assert bad.size == 0, f"{mesh}, axis {IR.AXIS_NAMES[axis]}: {bad.size} points differ, first {bad[:5]}: {p[bad[:5]]}, winding {w[bad[:5]]}"
    # the cases are not empty: both verdicts occur, under vertices too; the nested mesh reaches its deeper counts
    assert 50 <= got[:600].sum() <= 550 and 5 <= got[600:].sum() <= 95
    assert cr.max() >= (4 if mesh == "nested" else 2) and cr.min() == 0        # (the perturbed blob is not convex)
    if mesh == "nested":
        assert (np.rint(w) == 2).sum() >= 10 and (got[np.rint(w) == 2] == 0).all()      # inside the inner shell: outside


def test_cube_grid_on_all_six_axes():
    V, tri = IR.cube()
    assert V.shape == (8, 3) and tri.shape == (12, 3) and set(np.unique(V)) == {0.0, 2.0}
    assert abs(IR.winding_number(np.array([[1.0, 0.7, 0.4]]), V, tri)[0] - 1.0) < 1e-9                # closed, outward
    p = IR.cube_grid()
    assert p.shape == (125, 3)
    interior, outside = IR.cube_grid_classes(p)
    assert interior.sum() == 27 and outside.sum() == 50
    for axis in IR.AXES:
        got = IR.inside(IR.crossings(p, V, tri, axis))
        assert (got[interior] == 1).all(), f"axis {IR.AXIS_NAMES[axis]}: interior points outside: {p[interior & (got == 0)]}"
        assert (got[outside] == 0).all(), f"axis {IR.AXIS_NAMES[axis]}: outer points inside: {p[outside & (got == 1)]}"


def test_a_plain_hit_count_is_wrong_under_a_face_diagonal():
    V, tri = IR.cube()
    T = V[tri.astype(np.int64)]
    p = IR.cube_grid()
    interior, _ = IR.cube_grid_classes(p)
    for axis in IR.AXES:
        k, _, a, b = IR.axis_parts(axis)
        diag = interior & (p[:, a] == p[:, b])                  # under the face's diagonal from (0,0) to (2,2)
        assert diag.sum() == 9
        q = p[diag]
        o, d = q, (q + DIRS[axis]).astype(F32)
        hits = MH.totals(RR.pairs(o, d, T), *RR.bounds(o, d))
        assert (hits == 2).all(), hits                           # both triangles at the diagonal accept the ray ...
        assert ((hits & 1) == 0).all()                           # ... so its parity calls an interior point outside
        cr = IR.crossings(q, V, tri, axis)
        assert (cr == 1).all(), cr                               # the crossing rule claims the point for one of them


def test_non_finite_points_and_non_candidates_count_nothing():
    V, tri = IR.degenerate()
    cand = IR.candidates(V, tri)
    assert (~cand).sum() == 3 and cand[:512].all()
    p = np.concatenate([IR.uniform_points(V, 300, 3), IR.nonfinite_points()])
    Vb, trib = IR.blob()
    for axis in IR.AXES:
        k = axis >> 1
        cr = IR.crossings(p, V, tri, axis)
        assert (cr[-6:] == 0).all()
        # a triangle in the plane (coordinate j constant) is edge-on to the other two axes: along those it never
        # counts, so there the count is that of the blob with the other planes' triangles
        keep = np.zeros(len(tri), bool)
        keep[:512] = True
        keep[512 + 3 + 2 * k:512 + 3 + 2 * k + 2] = True          # the two triangles in a plane of constant coordinate k
        keep[-1] = k == 1                                        # the one at vertex 5 lies in a plane of constant y
        assert np.array_equal(cr, IR.crossings(p, V, tri[keep], axis)), IR.AXIS_NAMES[axis]
        assert not np.array_equal(cr, IR.crossings(p, Vb, trib, axis))          # (the face-on ones do count)
    assert IR.crossings(p, V, np.zeros((0, 3), np.uint32), 4).sum() == 0


def test_the_columns_are_thin():
    """The mean number of triangles whose acceptance-box column (the box across the axis, and not wholly behind the
    point along it) holds a point: below nt / 16 on the blob, so the GPU test's cap of nt / 4 evaluations per point
    has room for the leaves' other triangles."""
    V, tri = IR.blob()
    T = V[tri.astype(np.int64)]
    nt = len(tri)
    boxes = [bvh_acceptance_box(t) for t in T]
    assert all(st == 0 for st, _, _ in boxes)
    lo, hi = np.array([b[1] for b in boxes]), np.array([b[2] for b in boxes])
    assert (lo <= T.min(axis=1)).all() and (hi >= T.max(axis=1)).all()      # the boxes hold the vertices
    p = IR.uniform_points(V, 1024, 60)
    for axis in IR.AXES:
        k, sg, a, b = IR.axis_parts(axis)
        col = ((p[:, None, a] >= lo[None, :, a]) & (p[:, None, a] <= hi[None, :, a])
               & (p[:, None, b] >= lo[None, :, b]) & (p[:, None, b] <= hi[None, :, b]))
        col &= (p[:, None, k] <= hi[None, :, k]) if sg > 0 else (p[:, None, k] >= lo[None, :, k])
        mean = col.sum(axis=1).mean()
        print(f"axis {IR.AXIS_NAMES[axis]}: {mean:.2f} triangles per column of {nt}")
        assert mean < nt / 16
