"""The box-overlap expectation (tests/_box_overlap_ref.py, the numpy restatement of include/raytracert.h) against
exact rational clipping of the triangle by the box, on the CPU.

On the lattice (every coordinate a multiple of 1/16 in [-3, 3]) all of the restatement's arithmetic is exact: the
centre and half extent are multiples of 1/32, the products multiples of 2^-10 below 2^7 and the plane's sums
multiples of 2^-15 below 2^13, so the separating-axis verdict must equal the clipped polygon's on every pair. On
generic binary32 coordinates c, h and v_j each round once, a combined error of at most about 2^-22 M for a pair whose
largest coordinate magnitude is M; the verdict must lie between the exact verdicts of the box shrunk and grown by
16 times that, 2^-18 M, on every pair.
"""
from fractions import Fraction

import numpy as np

import _box_overlap_ref as BR
import _inside_ref as IR

F32 = np.float32
F64 = np.float64


def test_the_header_states_what_is_restated():
    """The restatement follows include/raytracert.h: the entry's comment must carry the definition's operations."""
    import re

    from raytracert_amd import _capi
    text = open(_capi.HEADER_PATH).read()
    start = text.index("The triangles that meet each axis-aligned query box")
    doc = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("int rt_box_overlap_device(", start)])
    for phrase in ("record normal is not (0,0,0)", "xyz[tri_v[3 t + j]]", "NaN or infinite component", "lo_a > hi_a", "No contraction",
                   "c = (lo + hi) * 0.5f", "h = (hi - lo) * 0.5f", "v_j = V_j - c", "binary64",
                   "f_0 = v_1 - v_0, f_1 = v_2 - v_1, f_2 = v_0 - v_2", "p_j = f[b] * v_j[c] - f[c] * v_j[b]",
                   "r = h[b] * |f[c]| + h[c] * |f[b]|", "n[a] = f_0[b] * f_1[c] - f_0[c] * f_1[b]",
                   "d = (n[0] v_0[0] + n[1] v_0[1]) + n[2] v_0[2]", "r = (h[0] |n[0]| + h[1] |n[1]|) + h[2] |n[2]|",
                   "separated if d > r or d < -r", "needs no margin", "2^-18"):
        assert phrase in doc, phrase


def _pairs(M, lo, hi, V, tri, grow_of=None):
    """The exact checker on every box x candidate triangle pair: [n, nt] bool (and with grow_of(i, t) -> margin,
    the verdicts with the box shrunk and grown by it)."""
    T = V[tri.astype(np.int64)]
    n, nt = M.shape
    if grow_of is None:
        return np.array([[BR.exact_overlap(lo[i], hi[i], T[t]) for t in range(nt)] for i in range(n)])
    shrunk, grown = np.zeros((n, nt), bool), np.zeros((n, nt), bool)
    for i in range(n):
        for t in range(nt):
            g = grow_of(i, t)
            shrunk[i, t] = BR.exact_overlap(lo[i], hi[i], T[t], -g)
            grown[i, t] = BR.exact_overlap(lo[i], hi[i], T[t], g)
    return shrunk, grown


def _lattice_set(seed, nt=60, nb=50):
    """nt lattice triangles (candidates) around random centres and nb lattice boxes, a third of the boxes with a
    face through a coordinate of a triangle's vertex."""
    rng = np.random.default_rng(seed)
    ctr = rng.integers(-32, 33, (nt, 1, 3))
    T = np.clip(ctr + rng.integers(-16, 17, (nt, 3, 3)), -48, 48).astype(F64) / 16.0
    V = np.ascontiguousarray(T.reshape(-1, 3), F32)
    tri = np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3)
    keep = IR.candidates(V, tri)
    tri = np.ascontiguousarray(tri[keep])
    a = rng.integers(-40, 41, (nb, 3))
    b = np.clip(a + rng.integers(0, 25, (nb, 3)), -48, 48)
    lo, hi = a.astype(F64) / 16.0, b.astype(F64) / 16.0
    for i in range(0, nb, 3):                                    # a face on a vertex coordinate
        v = V[tri[rng.integers(0, len(tri)), rng.integers(0, 3)]]
        ax = rng.integers(0, 3)
        if rng.integers(0, 2):
            hi[i, ax] = v[ax]
            lo[i, ax] = min(lo[i, ax], hi[i, ax])
        else:
            lo[i, ax] = v[ax]
            hi[i, ax] = max(hi[i, ax], lo[i, ax])
        others = [c for c in range(3) if c != ax]                # ... and the box around the vertex across
        lo[i, others] = np.minimum(lo[i, others], v[others])
        hi[i, others] = np.maximum(hi[i, others], v[others])
    return np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32), V, tri


def test_lattice_pairs_equal_exact_clipping():
    pairs = overlapping = touching = 0
    for seed in (1, 2):
        lo, hi, V, tri = _lattice_set(seed)
        assert (np.abs(V) <= 3).all() and (V * 16 == np.round(V * 16)).all() and (lo * 16 == np.round(lo * 16)).all()
        M = BR.overlap_matrix(lo, hi, V, tri)
        E = _pairs(M, lo, hi, V, tri)
        bad = np.argwhere(M != E)
        assert len(bad) == 0, f"seed {seed}: {len(bad)} pairs differ from exact clipping, first (box, triangle) {bad[:5].tolist()}"
        T = V[tri.astype(np.int64)]
        pairs += M.size
        overlapping += int(M.sum())
        # touching or thin contact: gone when the box shrinks by a quarter of the lattice step
        touching += sum(not BR.exact_overlap(lo[i], hi[i], T[t], Fraction(-1, 64)) for i, t in np.argwhere(M))
    print(f"{pairs} lattice pairs, {overlapping} overlap, {touching} of them only by touching or thin contact")
    assert pairs >= 5000 and overlapping >= 300 and touching >= 36


def _generic_set(seed, shift, nt=40, nb=40):
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(-1, 1, (nt, 1, 3))
    T = ctr + rng.uniform(-0.6, 0.6, (nt, 3, 3)) * rng.choice([1.0, 0.05], (nt, 1, 1))
    V = np.ascontiguousarray((T + shift).reshape(-1, 3), F32)
    tri = np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri[IR.candidates(V, tri)])
    c = rng.uniform(-1.2, 1.2, (nb, 3)) + shift
    h = rng.uniform(0, 0.7, (nb, 3)) * rng.choice([1.0, 0.02], (nb, 1))
    lo, hi = (c - h).astype(F32), (c + h).astype(F32)
    for i in range(0, nb, 3):                                    # a face exactly on a vertex coordinate
        v = V[tri[rng.integers(0, len(tri)), rng.integers(0, 3)]]
        ax = rng.integers(0, 3)
        if rng.integers(0, 2):
            hi[i, ax] = v[ax]
            lo[i, ax] = min(lo[i, ax], hi[i, ax])
        else:
            lo[i, ax] = v[ax]
            hi[i, ax] = max(hi[i, ax], lo[i, ax])
        others = [k for k in range(3) if k != ax]
        lo[i, others] = np.minimum(lo[i, others], v[others] - F32(0.1))
        hi[i, others] = np.maximum(hi[i, others], v[others] + F32(0.1))
    return np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32), V, tri


def test_generic_binary32_pairs_are_bracketed():
    """exact(box shrunk by 2^-18 M) implies the restatement's overlap implies exact(box grown by 2^-18 M), on every
    pair; M is the pair's own largest coordinate magnitude. Around the origin and far from it (where centring rounds
    away more of the vertices' bits)."""
    pairs = overlapping = strict = 0
    for seed, shift in ((3, np.zeros(3)), (4, np.array([37.3, -91.7, 12.9])), (5, np.array([-1000.1, 3.3, 512.7]))):
        lo, hi, V, tri = _generic_set(seed, shift)
        T = V[tri.astype(np.int64)]
        M = BR.overlap_matrix(lo, hi, V, tri)

        def margin(i, t):
            m = max(np.abs(T[t]).max(), np.abs(lo[i]).max(), np.abs(hi[i]).max())
            return Fraction(float(m)) / 2 ** 18

        shrunk, grown = _pairs(M, lo, hi, V, tri, margin)
        missed, invented = np.argwhere(shrunk & ~M), np.argwhere(M & ~grown)
        assert len(missed) == 0, f"shift {shift}: overlap inside the shrunk box not reported, (box, triangle) {missed[:5].tolist()}"
        assert len(invented) == 0, f"shift {shift}: overlap reported outside the grown box, (box, triangle) {invented[:5].tolist()}"
        pairs += M.size
        overlapping += int(M.sum())
        strict += int(shrunk.sum())
    print(f"{pairs} generic pairs, {overlapping} overlap, {strict} inside the shrunk box")
    assert pairs >= 4000 and overlapping >= 200


def test_empty_boxes_point_boxes_and_zero_normal_triangles():
    V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [1, 1, 0]], F32)
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 6, 6]], np.uint32)       # a triangle, three collinear points, a point
    assert IR.candidates(V, tri).tolist() == [True, False, False]
    elo, ehi = BR.empty_boxes()
    assert not BR.box_valid(elo, ehi).any()
    big_lo, big_hi = np.full((len(elo), 3), -10, F32), np.full((len(elo), 3), 10, F32)
    assert BR.overlap_matrix(big_lo, big_hi, V, tri)[:, 0].all()                          # (the same rows, valid: all overlap)
    assert not BR.overlap_matrix(elo, ehi, V, tri).any()
    # point boxes: on a vertex, on an edge, inside the triangle, off its plane, beside it in its plane
    pts = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [1, 1, 0], [1, 1, 0.0625], [3, 3, 0], [-0.0625, 0, 0]], F32)
    M = BR.overlap_matrix(pts, pts, V, tri)
    assert M[:, 0].tolist() == [True, True, True, True, False, False, False]
    assert not M[:, 1:].any()                                    # zero normals: never, even where the box holds them
    whole = BR.overlap_matrix(np.full((1, 3), -1, F32), np.full((1, 3), 5, F32), V, tri)
    assert whole.tolist() == [[True, False, False]]
    # touching counts: a box whose face lies in the triangle's plane, one that ends at its vertex
    lo = np.array([[1, 1, 0], [-1, -1, -1], [4, 0, 0]], F32)
    hi = np.array([[2, 2, 1], [0, 0, 0], [5, 1, 1]], F32)
    assert BR.overlap_matrix(lo, hi, V, tri)[:, 0].all()
    for i in range(3):
        assert BR.exact_overlap(lo[i], hi[i], V[tri[0].astype(np.int64)])


def test_lists_counts_and_paging():
    V, tri = IR.blob()
    lo, hi = BR.mesh_boxes(V)
    assert len(lo) >= 1024 + 300
    M = BR.overlap_matrix(lo, hi, V, tri)
    m_all = M.sum(axis=1)
    whole = int(np.argmax(m_all))
    assert m_all[whole] == len(tri) > 16                         # the all-containing box
    for k in (1, 4, 16):
        tris, nf, m = BR.lists(M, k)
        assert np.array_equal(m, m_all) and np.array_equal(nf, np.minimum(m_all, k))
        assert ((tris >= 0).sum(axis=1) == nf).all()
        filled = np.where(tris >= 0, tris, np.iinfo(np.int32).max)
        assert (np.diff(filled, axis=1) >= 0).all() and (np.diff(tris, axis=1)[(tris[:, 1:] >= 0)] > 0).all()
    # paging through the crowded box with after = the last index received gives every candidate once, in order
    k, after, got = 16, np.full(len(lo), -1, np.int64), []
    for _ in range(len(tri) // k + 2):
        tris, nf, m = BR.lists(M, k, after)
        if nf[whole] == 0:
            break
        got += tris[whole, :nf[whole]].tolist()
        after = np.where(nf > 0, tris[np.arange(len(lo)), np.maximum(nf, 1) - 1], after)
    assert got == np.flatnonzero(M[whole]).tolist() and len(got) == len(tri)
    assert m[whole] == 0 and (tris[whole] == -1).all()
