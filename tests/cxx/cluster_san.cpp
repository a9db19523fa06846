// Host-code sanitizer driver for the agglomerative builder (bvh.cpp build_cluster, bvh_cost), built by hand
// with tests/sanitize.mk's flags:
//   g++ $(CXXFLAGS of tests/sanitize.mk) -o cluster_san raytracert_amd/csrc/scene_loader.cpp \
//       raytracert_amd/csrc/obj_parallel.cpp raytracert_amd/csrc/bvh.cpp tests/cxx/cluster_san.cpp
//   cluster_san <obj>...     "ok <file> <triangles> <depth> <iterations> <cost>" per file, exit 0; a
//                            sanitizer report aborts
// Per file: build (validates; a second build has the same digest; nodes4 equals a remake from nodes4f; the
// cost is below the Morton tree's or equal), a refit after x += 0.03 sin(7y + 1), z += 0.03 cos(5x)
// (validates), a rebuild from the moved vertices (validates), a build with RTAMD_LBVH_MAX_DEPTH 3 (falls back
// with the depth reason unless the tree is that shallow), and 2,500 copies of the first triangle (the XOR
// tie rule: 12 iterations). Without arguments: only the copies, of a built-in triangle.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_internal.h"

using namespace rt;

static int copies(const float tri[9], int n, int want_iters) {
    HostScene c;
    c.mats.emplace_back();
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < 3; ++j) {
            for (int a = 0; a < 3; ++a) c.verts.push_back(tri[3 * j + a]);
            c.tris.push_back(static_cast<uint32_t>(3 * k + j));
        }
    c.tri_mat.assign(n, 0);
    compute_face_normals(c);
    std::vector<TriRec> recs;
    build_tri_records(c, recs);
    HostBvh h;
    std::string err;
    int32_t iters = 0, why = 0;
    if (build_cluster(c, recs, h, &iters, &why) != RT_OK || validate_bvh(c, recs, h, err) != RT_OK) {
        std::printf("copies invalid: %s (reason %d)\n", err.c_str(), why);
        return 1;
    }
    if (want_iters && iters != want_iters) { std::printf("copies: %d iterations, expected %d\n", iters, want_iters); return 1; }
    std::printf("ok copies %d depth %d iterations %d\n", n, h.depth, iters);
    return 0;
}

int main(int argc, char **argv) {
    int bad = 0;
    const float builtin[9] = {-0.5f, -0.4f, 0.1f, 0.6f, -0.3f, 0.0f, 0.1f, 0.7f, -0.2f};
    bad |= copies(builtin, 2500, 12);
    bad |= copies(builtin, 3, 0);
    bad |= copies(builtin, 2, 0);
    for (int f = 1; f < argc; ++f) {
        const char *path = argv[f];
        HostScene s;
        std::string err;
        if (load_obj(path, s, err) != RT_OK) { std::printf("unreadable %s\n", path); bad = 1; continue; }
        std::vector<TriRec> recs;
        build_tri_records(s, recs);
        HostBvh h, h2, lb;
        int32_t iters = 0, why = 0, iters2 = 0;
        if (build_cluster(s, recs, h, &iters, &why) != RT_OK) { std::printf("cluster fell back %s (reason %d)\n", path, why); bad = 1; continue; }
        if (validate_bvh(s, recs, h, err) != RT_OK) { std::printf("cluster invalid %s: %s\n", path, err.c_str()); bad = 1; }
        const uint64_t d0 = bvh_digest(h);
        if (build_cluster(s, recs, h2, &iters2, nullptr) != RT_OK || bvh_digest(h2) != d0 || iters2 != iters) { std::printf("not deterministic %s\n", path); bad = 1; }
        if (nodes4_from_nodes4f(h2) != RT_OK || bvh_digest(h2) != d0) { std::printf("nodes4 remake differs %s\n", path); bad = 1; }
        const double cost = bvh_cost(h);
        if (build_lbvh(s, recs, lb) == RT_OK && (lb.leaf_tris != h.leaf_tris || !(cost <= bvh_cost(lb)))) {
            std::printf("order or cost against the Morton tree %s: %g vs %g\n", path, cost, bvh_cost(lb));
            bad = 1;
        }
        setenv("RTAMD_LBVH_MAX_DEPTH", "3", 1);
        const int rc = build_cluster(s, recs, h2, nullptr, &why);
        if (rc != (h.depth <= 3 ? RT_OK : kLbvhFallback) || (rc != RT_OK && why != RT_FALLBACK_DEPTH)) { std::printf("depth bound missed %s\n", path); bad = 1; }
        unsetenv("RTAMD_LBVH_MAX_DEPTH");
        HostScene moved = s;
        for (size_t i = 0; i < moved.verts.size() / 3; ++i) {
            float *v = &moved.verts[3 * i];
            const float x = v[0];
            v[0] = x + 0.03f * std::sin(7.0f * v[1] + 1.0f);
            v[2] = v[2] + 0.03f * std::cos(5.0f * x);
        }
        compute_face_normals(moved);
        build_tri_records(moved, recs);
        if (refit_bvh(moved, recs, h) == RT_OK && validate_bvh(moved, recs, h, err) != RT_OK) {
            std::printf("refit invalid %s: %s\n", path, err.c_str());
            bad = 1;
        }
        if (build_cluster(moved, recs, h2, nullptr, nullptr) == RT_OK && validate_bvh(moved, recs, h2, err) != RT_OK) {
            std::printf("rebuild invalid %s: %s\n", path, err.c_str());
            bad = 1;
        }
        if (!s.tri_mat.empty()) {
            float tri[9];
            for (int j = 0; j < 3; ++j)
                for (int a = 0; a < 3; ++a) tri[3 * j + a] = s.verts[3 * s.tris[j] + a];
            bad |= copies(tri, 70, 0);
        }
        std::printf("ok %s %zu %d %d %.6f\n", path, s.tri_mat.size(), h.depth, iters, cost);
    }
    return bad;
}
