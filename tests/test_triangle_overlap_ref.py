"""The triangle-overlap expectation (tests/_triangle_overlap_ref.py, the numpy restatement of include/raytracert.h)
against an exact integer test of the two closed triangles, on the CPU.

On the lattice (every coordinate a multiple of 1/16 in [-3, 3]) all of the restatement's arithmetic is exact: the
differences are multiples of 2^-4 below 2^3, the normals and edge cross products multiples of 2^-8 below 2^7, the
in-plane axes multiples of 2^-12 below 2^11 and the projections multiples of 2^-16 below 2^15, at most 31 significant
bits, so the separating-axis verdict must equal the exact one on every pair: generic pairs, pairs forced coplanar and
pairs that touch (a shared vertex, a shared edge, a vertex on the other's edge line). On generic binary32 coordinates
the binary64 products round at about 2^-53 of their magnitude, so a verdict that differs from the exact one needs a
pair within about 2^-40 of the largest coordinate of touching; random pairs are never that close and the sets below,
with fixed seeds, are equal to the exact test on every pair too. No pair is left out of any set.
"""
import numpy as np

import _inside_ref as IR
import _triangle_overlap_ref as TR

F32 = np.float32
F64 = np.float64


def test_the_header_states_what_is_restated():
    """The restatement follows include/raytracert.h: the entry's comment must carry the definition's operations."""
    import re

    from raytracert_amd import _capi
    text = open(_capi.HEADER_PATH).read()
    start = text.index("The triangles that meet each query triangle")
    doc = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("int rt_triangle_overlap_device(", start)])
    for phrase in ("record normal is not (0,0,0)", "V_j = xyz[tri_v[3 t + j]]", "NaN or infinite component is empty", "No contraction",
                   "qlo_a = min_j Q_j[a], qhi_a = max_j Q_j[a]", "every V_j[a] > qhi_a, or every V_j[a] < qlo_a", "binary64",
                   "u_j[a] = (double)Q_j[a] - (double)Q_0[a]", "v_j[a] = (double)V_j[a] - (double)Q_0[a]", "no binary32 centring",
                   "e_0 = u_1 - u_0, e_1 = u_2 - u_1, e_2 = u_0 - u_2", "[a] = x[b] * y[c] - x[c] * y[b]",
                   "n_Q = e_0 cross e_1", "n_V = f_0 cross f_1", "n_Q is exactly (0,0,0) is empty", "seventeen axes",
                   "the nine e_i cross f_j, the three n_Q cross e_i and the three n_V cross f_j",
                   "p_j = (w[0] u_j[0] + w[1] u_j[1]) + w[2] u_j[2]", "every p_i < every q_j", "every p_i > every q_j",
                   "touching is overlap", "a NaN separates nothing", "no margin", "2^-40",
                   "t == self_i or when any of tri_v[3 t .. 3 t + 2] equals any of tri_v[3 self_i .. 3 self_i + 2]",
                   "folded onto its own neighbour is therefore not reported"):
        assert phrase in doc, phrase


def _scene_of(T):
    """(V, tri) with every triangle of T [nt, 3, 3] on vertices of its own."""
    V = np.ascontiguousarray(np.asarray(T, F32).reshape(-1, 3))
    return V, np.arange(len(V), dtype=np.uint32).reshape(-1, 3)


def _diag_against_exact(A, B, what):
    """Pair i is (A[i], B[i]); the restatement's verdict of every pair against the exact one. Returns the verdicts."""
    A, B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
    V, tri = _scene_of(B)
    assert IR.candidates(V, tri).all() and TR.query_valid(A).all(), what
    got = np.array([TR.overlap_matrix(A[i:i + 1], V, tri[i:i + 1])[0, 0] for i in range(len(A))])
    exact = np.array([TR.exact_overlap(A[i], B[i]) for i in range(len(A))])
    bad = np.flatnonzero(got != exact)
    assert bad.size == 0, f"{what}: {bad.size} of {len(A)} pairs differ from the exact test, first {bad[:5].tolist()}: {A[bad[:1]]}, {B[bad[:1]]}"
    return got


def _lattice_triangles(rng, n, spread=16):
    """n non-degenerate lattice triangles (units of 1/16, within +-3)."""
    out = []
    while len(out) < n:
        ctr = rng.integers(-32, 33, (1, 3))
        t = np.clip(ctr + rng.integers(-spread, spread + 1, (3, 3)), -48, 48)
        if np.any(np.cross(t[1] - t[0], t[2] - t[0])):
            out.append(t)
    return np.array(out)


def _in_plane_lattice(rng, t):
    """A non-degenerate lattice triangle in the plane of lattice triangle t (integer combinations of its edges that
    stay within +-3), or None."""
    for _ in range(20):
        c = rng.integers(-2, 3, (3, 2))
        q = t[0] + c[:, :1] * (t[1] - t[0]) + c[:, 1:] * (t[2] - t[0])
        if np.abs(q).max() <= 48 and np.any(np.cross(q[1] - q[0], q[2] - q[0])):
            return q
    return None


def test_lattice_pairs_equal_the_exact_test():
    rng = np.random.default_rng(1)
    # generic: two lattice triangles near one another
    A = _lattice_triangles(rng, 1200)
    B = np.clip(A[:, :1] + rng.integers(-20, 21, (1200, 3, 3)), -48, 48)
    keep = np.array([bool(np.any(np.cross(b[1] - b[0], b[2] - b[0]))) for b in B])
    generic = _diag_against_exact(A[keep] / 16.0, B[keep] / 16.0, "generic lattice pairs")
    # coplanar: the second triangle an integer combination of the first one's edges
    A2, B2 = [], []
    for t in _lattice_triangles(rng, 1600, spread=6):
        q = _in_plane_lattice(rng, t)
        if q is not None:
            A2.append(q)
            B2.append(t)
    coplanar = _diag_against_exact(np.array(A2) / 16.0, np.array(B2) / 16.0, "coplanar lattice pairs")
    # touching: a shared vertex, a shared edge, a vertex on the other's edge line
    A3, B3 = [], []
    for i, t in enumerate(_lattice_triangles(rng, 1300, spread=8)):
        q = _lattice_triangles(rng, 1, spread=8)[0]
        kind = i % 3
        if kind == 0:
            q[rng.integers(0, 3)] = t[rng.integers(0, 3)]
        elif kind == 1:
            q[0], q[1] = t[1], t[2]
        else:                                                    # a vertex of q on the line of t's first edge
            q[0] = t[0] + rng.integers(-1, 3) * (t[1] - t[0])
        if np.abs(q).max() <= 48 and np.any(np.cross(q[1] - q[0], q[2] - q[0])):
            A3.append(q)
            B3.append(t)
    touching = _diag_against_exact(np.array(A3) / 16.0, np.array(B3) / 16.0, "touching lattice pairs")
    print(f"lattice pairs equal to the exact test: generic {len(generic)} ({int(generic.sum())} overlap), coplanar {len(coplanar)} "
          f"({int(coplanar.sum())}), touching {len(touching)} ({int(touching.sum())})")
    assert len(generic) >= 1000 and len(coplanar) >= 1000 and len(touching) >= 1000
    assert 100 <= generic.sum() <= len(generic) - 100 and 100 <= coplanar.sum() <= len(coplanar) - 100
    assert touching.sum() >= 800                                 # (shared vertices and edges always overlap)


def test_generic_binary32_pairs_equal_the_exact_test():
    """Around the origin and far from it: 1,500 pairs each, every pair."""
    total = overlapping = 0
    for seed, shift in ((3, np.zeros(3)), (4, np.array([37.0, -92.0, 13.0])), (5, np.array([-1000.0, 3.0, 513.0]))):
        rng = np.random.default_rng(seed)
        ctr = rng.uniform(-1, 1, (1500, 1, 3))
        A = (ctr + rng.uniform(-0.6, 0.6, (1500, 3, 3)) * rng.choice([1.0, 0.3], (1500, 1, 1)) + shift).astype(F32)
        B = (ctr + rng.uniform(-0.1, 0.1, (1500, 1, 3)) + rng.uniform(-0.6, 0.6, (1500, 3, 3)) + shift).astype(F32)
        got = _diag_against_exact(A, B, f"generic pairs around {shift.tolist()}")
        total += len(got)
        overlapping += int(got.sum())
    print(f"{total} generic binary32 pairs equal to the exact test, {overlapping} overlap")
    assert total == 4500 and 0.15 * total <= overlapping <= 0.85 * total      # (both verdicts well represented)


def _verdict(Q, T):
    V, tri = _scene_of([T])
    return bool(TR.overlap_matrix(np.asarray([Q], F32), V, tri)[0, 0])


def test_named_constructions():
    T = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    cases = {
        "shared vertex": ([[0, 0, 0], [-1, -1, 3], [-2, 1, 2]], True),
        "shared edge": ([[0, 0, 0], [4, 0, 0], [1, -1, 3]], True),
        "vertex on face": ([[1, 1, 0], [1, 1, 2], [2, 1, 3]], True),
        "vertex just above the face": ([[1, 1, 0.0625], [1, 1, 2], [2, 1, 3]], False),
        "edge crossing edge at a point": ([[2, -1, -1], [2, 1, 1], [2, -1, 3]], True),
        "edge passing an edge": ([[2, -1, -1], [2, -0.0625, 1], [2, -1, 3]], False),
        "piercing the face": ([[1, 1, -1], [1, 1, 1], [5, 5, 1]], True),
        "coplanar overlapping": ([[1, 1, 0], [6, 1, 0], [1, 6, 0]], True),
        "coplanar, one inside the other": ([[0.5, 0.5, 0], [1.5, 0.5, 0], [0.5, 1.5, 0]], True),
        "coplanar, the other inside": ([[-1, -1, 0], [9, -1, 0], [-1, 9, 0]], True),
        "coplanar disjoint": ([[3, 3, 0], [5, 3, 0], [3, 5, 0]], False),
        "coplanar disjoint, boxes overlapping": ([[2.5, 2.5, 0], [4, 2.5, 0], [2.5, 4, 0]], False),
        "coplanar, touching along the hypotenuse": ([[4, 0, 0], [4, 4, 0], [0, 4, 0]], True),
        "coplanar, touching at a vertex": ([[4, 0, 0], [6, 0, 0], [6, -2, 0]], True),
        "parallel planes": ([[0, 0, 0.5], [4, 0, 0.5], [0, 4, 0.5]], False),
        "equal to the scene triangle": (T, True),
        "equal, other vertex order": ([T[2], T[1], T[0]], True),
    }
    for what, (Q, want) in cases.items():
        assert _verdict(Q, T) is want, what
        assert TR.exact_overlap(np.array(Q, F32), np.array(T, F32)) is want, what + " (exact)"
        assert _verdict(T, Q) is want, what + ", swapped"


def test_empty_queries_and_zero_normal_triangles():
    V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [1, 1, 0]], F32)
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 6, 6]], np.uint32)       # a triangle, three collinear points, a point
    assert IR.candidates(V, tri).tolist() == [True, False, False]
    big = np.array([[[-10, -10, -10], [10, 10, 10], [10, -10, 10]]], F32)     # the plane x = z: through all of them
    assert TR.overlap_matrix(big, V, tri).tolist() == [[True, False, False]]
    nf = TR.nonfinite_queries()
    assert not np.isfinite(nf).all(axis=(1, 2)).any() and not TR.query_valid(nf).any()
    assert not TR.overlap_matrix(nf, V, tri).any()
    za = TR.zero_area_queries(V)
    assert all(TR.exact_degenerate(q) for q in za) and not TR.query_valid(za).any()
    assert not TR.overlap_matrix(za, V, tri).any()
    # a zero-area query on the triangle itself: still empty (points and segments have other entries)
    on = np.array([[[1, 1, 0], [1, 1, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [2, 2, 0]]], F32)
    assert not TR.overlap_matrix(on, V, tri).any()


def test_self_and_after_semantics():
    V, tri = IR.blob()
    nt = len(tri)
    Q = V[tri.astype(np.int64)]
    M = TR.overlap_matrix(Q, V, tri)
    assert M[np.arange(nt), np.arange(nt)].all()                 # every triangle meets itself
    shares = np.array([[len(set(tri[i].tolist()) & set(tri[t].tolist())) > 0 for t in range(nt)] for i in range(nt)])
    assert (M & shares).sum() == shares.sum()                    # ... and every neighbour (touching is overlap)
    assert (shares.sum(axis=1) >= 10).all()                      # (itself, three across edges, the fans around its vertices)
    idx = np.arange(nt)
    skip = TR.self_matrix(tri, idx, nt)
    assert np.array_equal(skip, shares)
    assert not (M & ~skip).any()                                 # a closed surface that does not cut itself
    # values that name no triangle pass nothing over
    for s in (None, np.full(nt, -1), np.full(nt, nt), np.full(nt, np.iinfo(np.int32).min)):
        assert not TR.self_matrix(tri, s, nt).any()
    # the nested blobs do not meet; a copy of the blob moved by a quarter of its size does, and with
    # self = after = arange the pairs come once, at the lower index
    V2 = np.concatenate([V, (V + F32(0.25)).astype(F32)])
    tri2 = np.concatenate([tri, tri + np.uint32(len(V))])
    M2 = TR.overlap_matrix(V2[tri2.astype(np.int64)], V2, tri2) & ~TR.self_matrix(tri2, np.arange(2 * nt), 2 * nt)
    assert np.array_equal(M2, M2.T) and M2.any() and not M2[:nt, :nt].any() and not M2[nt:, nt:].any()
    tris, nf, m = TR.lists(M2, 16, np.arange(2 * nt))
    pairs = {(i, int(t)) for i in range(2 * nt) for t in tris[i] if t >= 0}
    assert (m <= 16).all() and all(i < t for i, t in pairs)
    assert pairs == {(int(i), int(t)) for i, t in np.argwhere(np.triu(M2))}
    assert len(pairs) == M2.sum() // 2 > 50


def test_lists_counts_and_paging():
    V, tri = IR.degenerate()                                     # (a plane cuts at most 64 of the plain blob's 512 triangles)
    Q = TR.mesh_queries(V, tri)
    assert 1250 <= len(Q) <= 1400
    M = TR.overlap_matrix(Q, V, tri)
    m_all = M.sum(axis=1)
    whole = int(np.argmax(m_all))
    assert whole == 1024 and m_all[whole] > 16 * 4               # the spanning triangle
    assert (m_all[-10:] == 0).all() and (m_all == 0).sum() >= 50 and (m_all > 0).sum() >= 300
    assert (m_all[1025:1075] >= 10).all()                        # a copy of a scene triangle meets it and its neighbours
    assert (m_all[1125:1225] >= 1).all()                         # a shared vertex or edge
    for k in (1, 4, 16):
        tris, nf, m = TR.lists(M, k)
        assert np.array_equal(m, m_all) and np.array_equal(nf, np.minimum(m_all, k))
        assert ((tris >= 0).sum(axis=1) == nf).all()
        filled = np.where(tris >= 0, tris, np.iinfo(np.int32).max)
        assert (np.diff(filled, axis=1) >= 0).all() and (np.diff(tris, axis=1)[(tris[:, 1:] >= 0)] > 0).all()
    k, after, got = 16, np.full(len(Q), -1, np.int64), []
    for _ in range(len(tri) // k + 2):
        tris, nf, m = TR.lists(M, k, after)
        if nf[whole] == 0:
            break
        got += tris[whole, :nf[whole]].tolist()
        after = np.where(nf > 0, tris[np.arange(len(Q)), np.maximum(nf, 1) - 1], after)
    assert got == np.flatnonzero(M[whole]).tolist() and len(got) == m_all[whole]
    assert m[whole] == 0 and (tris[whole] == -1).all()
    # step 1 alone already leaves the small queries few candidates
    assert TR.step1_survivors(Q[:1024], V, tri).sum(axis=1).mean() < len(tri) / 16
