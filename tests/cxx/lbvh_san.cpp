// Host-code sanitizer driver for the Morton-order builder (bvh.cpp build_lbvh, nodes4_from_nodes4f), built
// by hand with tests/sanitize.mk's flags:
//   g++ $(CXXFLAGS of tests/sanitize.mk) -o lbvh_san raytracert_amd/csrc/scene_loader.cpp \
//       raytracert_amd/csrc/obj_parallel.cpp raytracert_amd/csrc/bvh.cpp tests/cxx/lbvh_san.cpp
//   lbvh_san <obj>...     "ok <file> <triangles> <depth>" per file, exit 0; a sanitizer report aborts
// Per file: build (validates; a second build has the same digest; nodes4 equals a remake from nodes4f), a
// refit after x += 0.03 sin(7y + 1), z += 0.03 cos(5x) (validates), a build with RTAMD_LBVH_MAX_DEPTH 3
// (falls back unless the tree is that shallow), and 70 copies of the first triangle (the tie-break path).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_internal.h"

using namespace rt;

int main(int argc, char **argv) {
    int bad = 0;
    for (int f = 1; f < argc; ++f) {
        const char *path = argv[f];
        HostScene s;
        std::string err;
        if (load_obj(path, s, err) != RT_OK) { std::printf("unreadable %s\n", path); bad = 1; continue; }
        std::vector<TriRec> recs;
        build_tri_records(s, recs);
        HostBvh h, h2;
        if (build_lbvh(s, recs, h) != RT_OK) { std::printf("lbvh fell back %s\n", path); bad = 1; continue; }
        if (validate_bvh(s, recs, h, err) != RT_OK) { std::printf("lbvh invalid %s: %s\n", path, err.c_str()); bad = 1; }
        const uint64_t d0 = bvh_digest(h);
        if (build_lbvh(s, recs, h2) != RT_OK || bvh_digest(h2) != d0) { std::printf("not deterministic %s\n", path); bad = 1; }
        if (nodes4_from_nodes4f(h2) != RT_OK || bvh_digest(h2) != d0) { std::printf("nodes4 remake differs %s\n", path); bad = 1; }
        setenv("RTAMD_LBVH_MAX_DEPTH", "3", 1);
        if (build_lbvh(s, recs, h2) != (h.depth <= 3 ? RT_OK : kLbvhFallback)) { std::printf("depth bound missed %s\n", path); bad = 1; }
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
        if (!s.tri_mat.empty()) {
            HostScene c;
            c.mats = s.mats;
            for (int k = 0; k < 70; ++k)
                for (int j = 0; j < 3; ++j) {
                    for (int a = 0; a < 3; ++a) c.verts.push_back(s.verts[3 * s.tris[j] + a]);
                    c.tris.push_back(static_cast<uint32_t>(3 * k + j));
                }
            c.tri_mat.assign(70, s.tri_mat[0]);
            compute_face_normals(c);
            build_tri_records(c, recs);
            if (build_lbvh(c, recs, h2) != RT_OK || validate_bvh(c, recs, h2, err) != RT_OK) { std::printf("copies invalid %s: %s\n", path, err.c_str()); bad = 1; }
        }
        std::printf("ok %s %zu %d\n", path, s.tri_mat.size(), h.depth);
    }
    return bad;
}
