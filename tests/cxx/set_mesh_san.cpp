// Host-code sanitizer driver for rt_scene_set_mesh on host-only scenes (rt_capi.cpp's host path over
// scene_loader.cpp and bvh.cpp), a stand-alone program over the C ABI. Built by hand with tests/sanitize.mk's
// flags given to the host pass (the library's sources need the HIP headers, so the compiler is hipcc):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fno-fast-math -pthread \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1 \
//       -fsanitize=address,undefined -Iinclude -Iraytracert_amd/csrc -Iraytracert_amd/build -o set_mesh_san \
//       raytracert_amd/csrc/rt_kernels.hip -x hip raytracert_amd/csrc/rt_capi.cpp raytracert_amd/csrc/rt_comm.cpp \
//       -x none raytracert_amd/csrc/scene_loader.cpp raytracert_amd/csrc/obj_parallel.cpp raytracert_amd/csrc/bvh.cpp \
//       -x hip tests/cxx/set_mesh_san.cpp -ldl
//   set_mesh_san        "ok <builder> <mesh> <triangles>" per step, exit 0; a sanitizer report aborts
// No device is touched: every scene is RT_HOST_ONLY. Per builder one scene walks the chain of the CPU test
// (5 -> 2049 with degenerate and sliver triangles -> 3 -> 0 -> 65 -> an indexed grid with nt > nv); after each
// replacement its tree digest, order, export and validation equal a fresh rt_scene_create_ex's, then both
// take the same vertex update. A mesh with an index equal to nv is rejected and leaves the export unchanged.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "raytracert.h"
#include "raytracert_tune.h"

namespace {

struct Mesh {
    const char *name;
    std::vector<float> v;
    std::vector<uint32_t> t, m;
};

uint32_t g_state = 12345u;
float unit() {   // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return static_cast<float>(g_state >> 8) / 16777216.0f;
}

Mesh soup(const char *name, int n, bool mixed) {
    Mesh s{name, {}, {}, {}};
    for (int i = 0; i < n; ++i) {
        const float c[3] = {2 * unit() - 1, 2 * unit() - 1, 2 * unit() - 1};
        float p[3][3] = {{c[0] - 0.008f, c[1] - 0.006f, c[2] - 0.002f}, {c[0] + 0.008f, c[1] - 0.005f, c[2] + 0.002f},
                         {c[0], c[1] + 0.011f, c[2] + 0.001f}};
        const float draw = unit();
        if (mixed && draw < 0.1f) std::memcpy(p[2], p[0], sizeof p[0]);   // zero area: never accepted
        else if (mixed && draw < 0.2f)                                    // a sliver: tested by every query
            for (int k = 0; k < 3; ++k) p[2][k] = p[0][k] + 0.5f * (p[1][k] - p[0][k]) + (k == 1 ? 1e-6f : 0.0f);
        for (int j = 0; j < 3; ++j) {
            s.t.push_back(static_cast<uint32_t>(s.v.size() / 3));
            s.v.insert(s.v.end(), p[j], p[j] + 3);
        }
        s.m.push_back(static_cast<uint32_t>(i & 1));
    }
    return s;
}

Mesh grid(const char *name, int w, int h) {   // shared vertices: nt = 2 (w - 1)(h - 1) > nv = w h
    Mesh s{name, {}, {}, {}};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const float p[3] = {0.05f * x - 1.0f, 0.05f * y - 1.0f, 0.01f * static_cast<float>((x * 7 + y * 3) % 5)};
            s.v.insert(s.v.end(), p, p + 3);
        }
    for (int y = 0; y + 1 < h; ++y)
        for (int x = 0; x + 1 < w; ++x) {
            const uint32_t a = static_cast<uint32_t>(y * w + x), b = a + 1, c = a + static_cast<uint32_t>(w), d = c + 1;
            const uint32_t q[6] = {a, b, c, b, d, c};
            s.t.insert(s.t.end(), q, q + 6);
            s.m.push_back(0);
            s.m.push_back(1);
        }
    return s;
}

struct Dump {
    std::vector<float> v, n;
    std::vector<uint32_t> t, m, leaf, always;
    uint64_t digest = 0;
    int32_t info[RT_BVH_INFO_FIELDS] = {};
    bool operator==(const Dump &o) const {
        return v.size() == o.v.size() && (v.empty() || !std::memcmp(v.data(), o.v.data(), 4 * v.size())) && n.size() == o.n.size() &&
               (n.empty() || !std::memcmp(n.data(), o.n.data(), 4 * n.size())) && t == o.t && m == o.m && leaf == o.leaf &&
               always == o.always && digest == o.digest && !std::memcmp(info, o.info, sizeof info);
    }
};

bool dump(rt_scene *s, Dump &d) {
    int32_t nv = 0, nt = 0, nm = 0;
    if (rt_scene_info(s, &nv, &nt, &nm) != RT_OK) return false;
    d.v.assign(3 * static_cast<size_t>(nv), 0.0f);
    d.n.assign(3 * static_cast<size_t>(nt), 0.0f);
    d.t.assign(3 * static_cast<size_t>(nt), 0u);
    d.m.assign(static_cast<size_t>(nt), 0u);
    if (rt_scene_export(s, d.v.data(), d.t.data(), d.m.data(), nullptr, d.n.data()) != RT_OK) return false;
    if (rt_scene_bvh_digest(s, &d.digest) != RT_OK || rt_scene_bvh_info(s, d.info) != RT_OK) return false;
    d.leaf.assign(static_cast<size_t>(nt) + 1, 0u);
    d.always.assign(static_cast<size_t>(nt) + 1, 0u);
    int64_t nl = 0, na = 0;
    if (rt_scene_bvh_order(s, d.leaf.data(), static_cast<int64_t>(d.leaf.size()), &nl, d.always.data(),
                           static_cast<int64_t>(d.always.size()), &na) != RT_OK)
        return false;
    d.leaf.resize(static_cast<size_t>(nl));
    d.always.resize(static_cast<size_t>(na));
    return rt_scene_bvh_validate(s) == RT_OK;
}

}  // namespace

int main() {
    const rt_material mats[2] = {{{0.8f, 0.2f, 0.2f}, {0.1f, 0.1f, 0.1f}, {0.5f, 0.5f, 0.5f}, 20.0f, 1.0f, 1.0f, 2, 0},
                                 {{0.2f, 0.8f, 0.2f}, {0.1f, 0.1f, 0.1f}, {0.3f, 0.3f, 0.3f}, 5.0f, 1.3f, 0.5f, 2, 0x20}};
    const std::vector<Mesh> chain = {soup("soup5", 5, false),  soup("mixed2049", 2049, true), soup("soup3", 3, false),
                                     Mesh{"empty", {}, {}, {}}, soup("soup65", 65, false),     grid("grid", 40, 30)};
    const Mesh first = soup("soup9", 9, false);
    const char *names[3] = {"sah", "lbvh", "cluster"};
    int bad = 0;
    for (int32_t builder = RT_BUILD_SAH; builder <= RT_BUILD_CLUSTER; ++builder) {
        rt_scene *sc = nullptr;
        if (rt_scene_create_ex(first.v.data(), static_cast<int32_t>(first.v.size() / 3), first.t.data(), first.m.data(),
                               static_cast<int32_t>(first.m.size()), mats, 2, RT_HOST_ONLY, builder, &sc) != RT_OK) {
            std::printf("create failed: %s\n", rt_last_error_string());
            return 1;
        }
        for (const Mesh &mesh : chain) {
            const int32_t nv = static_cast<int32_t>(mesh.v.size() / 3), nt = static_cast<int32_t>(mesh.m.size());
            int32_t outcome = -1;
            if (rt_scene_set_mesh(sc, mesh.v.data(), nv, mesh.t.data(), mesh.m.data(), nt, &outcome) != RT_OK) {
                std::printf("set_mesh failed %s %s: %s\n", names[builder], mesh.name, rt_last_error_string());
                bad = 1;
                continue;
            }
            rt_scene *fresh = nullptr;
            if (rt_scene_create_ex(mesh.v.data(), nv, mesh.t.data(), mesh.m.data(), nt, mats, 2, RT_HOST_ONLY, builder, &fresh) != RT_OK) {
                std::printf("fresh failed %s %s: %s\n", names[builder], mesh.name, rt_last_error_string());
                bad = 1;
                continue;
            }
            Dump a, b;
            if (!dump(sc, a) || !dump(fresh, b) || !(a == b)) { std::printf("differs from fresh %s %s\n", names[builder], mesh.name); bad = 1; }
            if (outcome < RT_UPDATED_REBUILT || outcome > RT_UPDATED_REBUILT_CLUSTER) { std::printf("outcome %d\n", outcome); bad = 1; }
            if (nv) {   // the same vertex update on both: scale and shift keep every class
                std::vector<float> moved(mesh.v);
                for (size_t i = 0; i < moved.size(); ++i) moved[i] = moved[i] * 1.25f + (i % 3 == 0 ? 0.05f : i % 3 == 1 ? -0.1f : 0.3f);
                int32_t oa = -1, ob = -1;
                if (rt_scene_update_vertices(sc, moved.data(), nv, RT_UPDATE_AUTO, &oa) != RT_OK ||
                    rt_scene_update_vertices(fresh, moved.data(), nv, RT_UPDATE_AUTO, &ob) != RT_OK || oa != ob || !dump(sc, a) ||
                    !dump(fresh, b) || !(a == b)) {
                    std::printf("update differs from fresh %s %s\n", names[builder], mesh.name);
                    bad = 1;
                }
            }
            if (nt) {   // rejected: one index equal to nv, one material equal to the table's size; the scene stays
                Dump before, after;
                dump(sc, before);
                std::vector<uint32_t> t(mesh.t), m(mesh.m);
                t[t.size() / 2] = static_cast<uint32_t>(nv);
                m[m.size() / 2] = 2;
                if (rt_scene_set_mesh(sc, mesh.v.data(), nv, t.data(), mesh.m.data(), nt, &outcome) != RT_E_PARSE ||
                    rt_scene_set_mesh(sc, mesh.v.data(), nv, mesh.t.data(), m.data(), nt, &outcome) != RT_E_PARSE || !dump(sc, after) ||
                    !(before == after)) {
                    std::printf("rejection wrong %s %s\n", names[builder], mesh.name);
                    bad = 1;
                }
            }
            rt_scene_destroy(fresh);
            std::printf("ok %s %s %d\n", names[builder], mesh.name, nt);
        }
        rt_scene_destroy(sc);
    }
    return bad;
}
