/* raytracert.hpp — C++ host layer over librtamd.so (include/raytracert.h) with the names and
 * argument meaning of the reference's tracer interface (CG_Project/raytracing.h), so a host that
 * calls init / performRayTracing / trace / getMaterial keeps its code and gets the MI355X path.
 *
 *   reference (CG_Project/)                      here (namespace rtamd)
 *   extern Mesh MyMesh; normals (raytracing.h:8)  RayTracer holds the scene (rt_scene)
 *   MyLightPositions, MyCameraPosition,           RayTracer members of the same names
 *   WindowSize_X/Y, pixelfactorX/Y, max_lvl,
 *   Ambient ... Refraction (raytracing.cpp:15-29)
 *   void init(char*)              :19, .cpp:42-73  RayTracer::init — load OBJ/MTL, face normals,
 *                                                  light 0 = the camera position
 *   Material getMaterial(int)     :27, .cpp:373    RayTracer::getMaterial
 *   Vec3Df trace(o, d, lvl)       :30, .cpp:381    RayTracer::trace (max_lvl - lvl levels left)
 *   Vec3Df performRayTracing(o,d) :33, .cpp:410    RayTracer::performRayTracing (+ a batched form)
 *   intersectMesh (.cpp:161-192)                   RayTracer::intersectMesh
 *   key 'd' debug shot (.cpp:493-510)              RayTracer::debugTrace
 *   key 'r' frame loop (main.cpp:340-411)          RayTracer::render (+ writeImage)
 *
 * Vec3Df is layout-compatible with the reference's Vec3D<float> (three floats, Vec3D.h:272,291)
 * and Material exposes the accessors of mesh.h:10-125. Failures throw rtamd::Error with
 * rt_last_error_string() (the reference has no error path: a missing OBJ crashes, mesh.cpp:329).
 * Header-only; link with -lrtamd. */
#ifndef RAYTRACERT_HPP_
#define RAYTRACERT_HPP_

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "raytracert.h"

namespace rtamd {

class Error : public std::runtime_error {
  public:
    Error(int code, const std::string &what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }

  private:
    int code_;
};

inline void check(int rc) {
    if (rc != RT_OK) throw Error(rc, rt_last_error_string());
}

struct Vec3Df {
    float p[3];
    Vec3Df() : p{0.0f, 0.0f, 0.0f} {}
    Vec3Df(float x, float y, float z) : p{x, y, z} {}
    float &operator[](int i) { return p[i]; }
    const float &operator[](int i) const { return p[i]; }
    Vec3Df operator+(const Vec3Df &o) const { return Vec3Df(p[0] + o.p[0], p[1] + o.p[1], p[2] + o.p[2]); }
    Vec3Df operator-(const Vec3Df &o) const { return Vec3Df(p[0] - o.p[0], p[1] - o.p[1], p[2] - o.p[2]); }
    Vec3Df operator*(float f) const { return Vec3Df(p[0] * f, p[1] * f, p[2] * f); }
    bool operator==(const Vec3Df &o) const { return p[0] == o.p[0] && p[1] == o.p[1] && p[2] == o.p[2]; }
    static float dotProduct(const Vec3Df &a, const Vec3Df &b) { return a.p[0] * b.p[0] + a.p[1] * b.p[1] + a.p[2] * b.p[2]; }
};
static_assert(sizeof(Vec3Df) == 12, "Vec3Df must be three packed floats");
static_assert(sizeof(Vec3Df) == sizeof(rt_vec3), "Vec3Df and rt_vec3 share the layout");

// Material with the accessor names of the reference (mesh.h:10-125)
class Material {
  public:
    Material() : m_{} {}
    explicit Material(const rt_material &m) : m_(m) {}
    Vec3Df Kd() const { return Vec3Df(m_.Kd[0], m_.Kd[1], m_.Kd[2]); }
    Vec3Df Ka() const { return Vec3Df(m_.Ka[0], m_.Ka[1], m_.Ka[2]); }
    Vec3Df Ks() const { return Vec3Df(m_.Ks[0], m_.Ks[1], m_.Ks[2]); }
    float Ns() const { return m_.Ns; }
    float Ni() const { return m_.Ni; }
    float Tr() const { return m_.Tr; }
    int illum() const { return m_.illum; }
    bool has_Kd() const { return (m_.flags & RT_HAS_KD) != 0; }
    bool has_Ka() const { return (m_.flags & RT_HAS_KA) != 0; }
    bool has_Ks() const { return (m_.flags & RT_HAS_KS) != 0; }
    bool has_Ns() const { return (m_.flags & RT_HAS_NS) != 0; }
    bool has_Ni() const { return (m_.flags & RT_HAS_NI) != 0; }
    bool has_illum() const { return (m_.flags & RT_HAS_ILLUM) != 0; }
    bool has_Tr() const { return (m_.flags & RT_HAS_TR) != 0; }
    bool is_valid() const { return has_Kd() || has_Ka() || has_Ks() || has_Tr(); }   // mesh.h:55-56
    const rt_material &raw() const { return m_; }

  private:
    rt_material m_;
};

class RayTracer {
  public:
    // the reference's globals (raytracing.h:8-16, raytracing.cpp:15-29, main.cpp:130-138)
    std::vector<Vec3Df> MyLightPositions;
    Vec3Df MyCameraPosition{0.0f, 0.0f, 4.0f};
    unsigned int WindowSize_X = 800, WindowSize_Y = 800;
    unsigned int pixelfactorX = 3, pixelfactorY = 3;
    int max_lvl = 10;
    bool Ambient = true, Diffuse = true, Reflection = true, Shadows = true, Specular = true, Refraction = true;

    // device: a HIP device index, or RT_HOST_ONLY (loader and getMaterial only)
    explicit RayTracer(int device = 0) : device_(device) {}
    ~RayTracer() { rt_scene_destroy(scene_); }
    RayTracer(const RayTracer &) = delete;
    RayTracer &operator=(const RayTracer &) = delete;

    // init(char*), raytracing.cpp:42-73: loadMesh + calculateNormals, then light 0 = camera
    void init(const char *fileName) {
        rt_scene_destroy(scene_);
        scene_ = nullptr;
        check(rt_scene_load_obj(fileName ? fileName : "cube.obj", device_, &scene_));
        MyLightPositions.push_back(MyCameraPosition);
    }

    // Extension (the reference's mesh is fixed after init): new positions for MyMesh.vertices, same count
    // (rt_scene_update_vertices). True when the BVH was refitted, false when it had to be rebuilt; the
    // scene then renders as one loaded from the new vertices either way.
    bool updateVertices(const std::vector<Vec3Df> &vertices, bool rebuild = false) {
        int32_t outcome = RT_UPDATED_REBUILT;
        check(rt_scene_update_vertices(scene_, vertices.empty() ? nullptr : vertices[0].p, static_cast<int32_t>(vertices.size()),
                                       rebuild ? RT_UPDATE_REBUILD : RT_UPDATE_AUTO, &outcome));
        return outcome == RT_UPDATED_REFIT;
    }
    // Extension: MyMesh's vertices, triangles and triangle materials replaced, counts free to change
    // (rt_scene_set_mesh; triangles = 3 vertex indices each). The materials, builder and settings stay.
    // Returns the RT_UPDATED_REBUILT* value of the builder that made the new trees.
    int32_t setMesh(const std::vector<Vec3Df> &vertices, const std::vector<uint32_t> &triangles,
                    const std::vector<uint32_t> &triangleMaterials) {
        int32_t outcome = RT_UPDATED_REBUILT;
        check(rt_scene_set_mesh(scene_, vertices.empty() ? nullptr : vertices[0].p, static_cast<int32_t>(vertices.size()),
                                triangles.data(), triangleMaterials.data(), static_cast<int32_t>(triangleMaterials.size()), &outcome));
        return outcome;
    }
    // The same from device memory on the scene's device (rt_scene_set_mesh_device): float xyz[3 nv], uint32
    // tri_v[3 nt], uint32 tri_mat[nt]; d_counts: null, or a device int32[2] of live counts.
    int32_t setMeshDevice(const void *d_xyz, int32_t n_vertices, const void *d_tri_v, const void *d_tri_mat, int32_t n_triangles,
                          const void *d_counts = nullptr) {
        int32_t outcome = RT_UPDATED_REBUILT;
        check(rt_scene_set_mesh_device(scene_, d_xyz, n_vertices, d_tri_v, d_tri_mat, n_triangles, d_counts, &outcome));
        return outcome;
    }
    // The builder of later rebuilds (rt_scene_set_builder): RT_BUILD_SAH (the default), RT_BUILD_LBVH, the
    // Morton-order tree built on the GPU (same results, a far cheaper rebuild, somewhat slower frames), or
    // RT_BUILD_CLUSTER, the agglomerative tree built on the GPU (a little dearer to build, faster frames).
    void setBuilder(int32_t builder) { check(rt_scene_set_builder(scene_, builder)); }

    // getMaterial(int), raytracing.cpp:373-376
    Material getMaterial(int index) const {
        rt_material m;
        check(rt_get_material(scene_, index, &m));
        return Material(m);
    }

    // intersectMesh, raytracing.cpp:161-192: closest triangle index or -1, point in *intersectOut
    int intersectMesh(const Vec3Df &origin, const Vec3Df &dest, Vec3Df *intersectOut) const {
        int32_t idx = -1;
        Vec3Df I;
        check(rt_intersect_mesh(scene_, origin.p, dest.p, 1, &idx, I.p));
        if (intersectOut) *intersectOut = I;
        return idx;
    }

    // trace(origin, dest, lvl), raytracing.cpp:381-406: the chain below level lvl of max_lvl
    // (every level test is lvl < max_lvl with unit steps, so it is the max_lvl - lvl chain)
    Vec3Df trace(const Vec3Df &origin, const Vec3Df &dest, int lvl) {
        rt_params p = params();
        p.max_lvl = lvl >= max_lvl ? 0 : max_lvl - lvl;
        Vec3Df c;
        check(rt_trace_rays(scene_, &p, origin.p, dest.p, 1, c.p, nullptr));
        return c;
    }

    // performRayTracing, raytracing.cpp:410-416 (= trace(origin, dest, 0))
    Vec3Df performRayTracing(const Vec3Df &origin, const Vec3Df &dest) { return trace(origin, dest, 0); }

    // the same for many rays at once (the form the GPU wants)
    std::vector<Vec3Df> performRayTracing(const std::vector<Vec3Df> &origins, const std::vector<Vec3Df> &dests) {
        if (origins.size() != dests.size()) throw Error(RT_E_ARG, "origins/dests size mismatch");
        std::vector<Vec3Df> out(origins.size());
        rt_params p = params();
        check(rt_trace_rays(scene_, &p, origins.empty() ? nullptr : origins[0].p, dests.empty() ? nullptr : dests[0].p,
                            static_cast<int32_t>(origins.size()), out.empty() ? nullptr : out[0].p, nullptr));
        return out;
    }

    // Extensions: the same queries for rays that are already in device memory, results to device memory, on
    // the caller's hipStream_t with no host copy (rt_intersect_mesh_device, rt_occluded_device,
    // rt_trace_rays_device; ray_stride RT_RAYS_PACKED or RT_RAYS_PADDED, d_count may be null).
    void intersect_mesh_device(const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n, const void *d_count,
                               void *d_index_out, void *d_point_out, void *stream) {
        check(rt_intersect_mesh_device(scene_, d_origins, d_dests, ray_stride, n, d_count, d_index_out, d_point_out, stream));
    }
    void occluded_device(const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n, const void *d_count,
                         void *d_blocked_out, void *stream) {
        check(rt_occluded_device(scene_, d_origins, d_dests, ray_stride, n, d_count, d_blocked_out, stream));
    }
    // ... and within a per-ray distance range [tmin, tmax) (rt_closest_hit_range_device, rt_occluded_range_device:
    // d_tmin / d_tmax n device floats each or null, flags RT_RANGE_TO_DEST / RT_OCCLUDE_ANY_OPAQUE; d_hit_out
    // n x rt_hit, d_point_out may be null)
    void closest_hit_range_device(const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n, const void *d_count,
                                  const void *d_tmin, const void *d_tmax, uint32_t flags, void *d_hit_out, void *d_point_out,
                                  void *stream) {
        check(rt_closest_hit_range_device(scene_, d_origins, d_dests, ray_stride, n, d_count, d_tmin, d_tmax, flags, d_hit_out,
                                          d_point_out, stream));
    }
    void occluded_range_device(const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n, const void *d_count,
                               const void *d_tmin, const void *d_tmax, uint32_t flags, void *d_blocked_out, void *stream) {
        check(rt_occluded_range_device(scene_, d_origins, d_dests, ray_stride, n, d_count, d_tmin, d_tmax, flags, d_blocked_out,
                                       stream));
    }
    // ... and the first k hits of each ray in that range from one walk (rt_multi_hit_range_device: d_hits_out
    // n x k rt_hit, d_nhits_out n x int32 or null; flags RT_RANGE_TO_DEST / RT_MULTI_COUNT_ALL)
    void multi_hit_range_device(const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n, const void *d_count,
                                const void *d_tmin, const void *d_tmax, uint32_t flags, int32_t k, void *d_hits_out,
                                void *d_nhits_out, void *stream) {
        check(rt_multi_hit_range_device(scene_, d_origins, d_dests, ray_stride, n, d_count, d_tmin, d_tmax, flags, k, d_hits_out,
                                        d_nhits_out, stream));
    }
    // the nearest point of the mesh to each query point (rt_closest_point_device: d_hit_out n x rt_hit, d_point_out
    // 3n floats or null, d_rmax n search radii or null; flags 0)
    void closest_point_device(const void *d_points, int32_t point_stride, int32_t n, const void *d_count, const void *d_rmax,
                              uint32_t flags, void *d_hit_out, void *d_point_out, void *stream) {
        check(rt_closest_point_device(scene_, d_points, point_stride, n, d_count, d_rmax, flags, d_hit_out, d_point_out, stream));
    }
    // the k nearest triangles of each query point (rt_nearest_triangles_device: d_hits_out n x k rt_hit, d_nfound_out
    // n int32 or null, d_points_out n x k x 3 floats or null; flags: RT_NEAR_COUNT_ALL)
    void nearest_triangles_device(const void *d_points, int32_t point_stride, int32_t n, const void *d_count, const void *d_rmax,
                                  uint32_t flags, int32_t k, void *d_hits_out, void *d_nfound_out, void *d_points_out, void *stream) {
        check(rt_nearest_triangles_device(scene_, d_points, point_stride, n, d_count, d_rmax, flags, k, d_hits_out, d_nfound_out,
                                          d_points_out, stream));
    }
    // whether each query point has a triangle inside its radius (rt_within_radius_device: d_within_out n x uint8; flags 0)
    void within_radius_device(const void *d_points, int32_t point_stride, int32_t n, const void *d_count, const void *d_rmax,
                              uint32_t flags, void *d_within_out, void *stream) {
        check(rt_within_radius_device(scene_, d_points, point_stride, n, d_count, d_rmax, flags, d_within_out, stream));
    }
    // whether each query point is inside the mesh, by crossing parity along an axis (rt_point_inside_device: axis
    // RT_AXIS_POS_X .. RT_AXIS_NEG_Z, d_inside_out n x uint8, d_crossings_out n int32 or null; flags 0)
    void point_inside_device(const void *d_points, int32_t point_stride, int32_t n, const void *d_count, int32_t axis, uint32_t flags,
                             void *d_inside_out, void *d_crossings_out, void *stream) {
        check(rt_point_inside_device(scene_, d_points, point_stride, n, d_count, axis, flags, d_inside_out, d_crossings_out, stream));
    }
    // closest_point_device with the distance negative inside the mesh (rt_signed_distance_device: d_inside_out n x uint8
    // or null; flags 0)
    void signed_distance_device(const void *d_points, int32_t point_stride, int32_t n, const void *d_count, const void *d_rmax,
                                int32_t axis, uint32_t flags, void *d_hit_out, void *d_point_out, void *d_inside_out, void *stream) {
        check(rt_signed_distance_device(scene_, d_points, point_stride, n, d_count, d_rmax, axis, flags, d_hit_out, d_point_out,
                                        d_inside_out, stream));
    }
    // the triangles that meet each axis-aligned box, lowest indices first (rt_box_overlap_device: d_after n int32 or null,
    // d_tris_out n x k int32, d_nfound_out n int32 or null; flags: RT_BOX_COUNT_ALL)
    void box_overlap_device(const void *d_lo, const void *d_hi, int32_t box_stride, int32_t n, const void *d_count, const void *d_after,
                            uint32_t flags, int32_t k, void *d_tris_out, void *d_nfound_out, void *stream) {
        check(rt_box_overlap_device(scene_, d_lo, d_hi, box_stride, n, d_count, d_after, flags, k, d_tris_out, d_nfound_out, stream));
    }
    // whether a triangle meets each box (rt_box_occupied_device: d_occupied_out n x uint8; flags 0)
    void box_occupied_device(const void *d_lo, const void *d_hi, int32_t box_stride, int32_t n, const void *d_count, uint32_t flags,
                             void *d_occupied_out, void *stream) {
        check(rt_box_occupied_device(scene_, d_lo, d_hi, box_stride, n, d_count, flags, d_occupied_out, stream));
    }
    // the triangles that meet each query triangle, lowest indices first (rt_triangle_overlap_device: d_qtris 3 n vertices,
    // d_after and d_self n int32 or null, d_tris_out n x k int32, d_nfound_out n int32 or null; flags: RT_TRI_COUNT_ALL)
    void triangle_overlap_device(const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count, const void *d_after,
                                 const void *d_self, uint32_t flags, int32_t k, void *d_tris_out, void *d_nfound_out, void *stream) {
        check(rt_triangle_overlap_device(scene_, d_qtris, tri_stride, n, d_count, d_after, d_self, flags, k, d_tris_out, d_nfound_out,
                                         stream));
    }
    // whether a triangle meets each query triangle (rt_triangle_collides_device: d_collides_out n x uint8; flags 0)
    void triangle_collides_device(const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count, const void *d_self,
                                  uint32_t flags, void *d_collides_out, void *stream) {
        check(rt_triangle_collides_device(scene_, d_qtris, tri_stride, n, d_count, d_self, flags, d_collides_out, stream));
    }
    // the scene triangle nearest to each query triangle (rt_triangle_distance_device: d_rmax n floats, d_self n int32,
    // d_qpoint_out and d_point_out 3 n floats, each or null; d_hit_out n x rt_hit; flags 0)
    void triangle_distance_device(const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count, const void *d_rmax,
                                  const void *d_self, uint32_t flags, void *d_hit_out, void *d_qpoint_out, void *d_point_out, void *stream) {
        check(rt_triangle_distance_device(scene_, d_qtris, tri_stride, n, d_count, d_rmax, d_self, flags, d_hit_out, d_qpoint_out, d_point_out,
                                          stream));
    }
    // whether a scene triangle is within the radius of each query triangle (rt_triangle_within_device: d_within_out n x uint8)
    void triangle_within_device(const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count, const void *d_rmax,
                                const void *d_self, uint32_t flags, void *d_within_out, void *stream) {
        check(rt_triangle_within_device(scene_, d_qtris, tri_stride, n, d_count, d_rmax, d_self, flags, d_within_out, stream));
    }
    void perform_ray_tracing_device(const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n, void *d_rgb_out,
                                    void *stream, uint64_t counts[3] = nullptr) {
        rt_params p = params();
        check(rt_trace_rays_device(scene_, &p, d_origins, d_dests, ray_stride, n, d_rgb_out, stream, counts));
    }

    // the debug key 'd' (raytracing.cpp:493-510): every trace() of the ray's chain, and its colour
    std::vector<rt_debug_bounce> debugTrace(const Vec3Df &origin, const Vec3Df &dest, Vec3Df *color = nullptr) {
        std::vector<rt_debug_bounce> b(static_cast<size_t>(max_lvl) * 2 + 2);
        int32_t n = 0;
        Vec3Df c;
        rt_params p = params();
        check(rt_debug_trace(scene_, &p, origin.p, dest.p, b.data(), static_cast<int32_t>(b.size()), &n, c.p));
        b.resize(static_cast<size_t>(n) < b.size() ? static_cast<size_t>(n) : b.size());
        if (color) *color = c;
        return b;
    }

    // the 'r' key (main.cpp:340-411): WindowSize_X x WindowSize_Y bytes as Image::writeImage
    // writes them. corners = the four produceRay results origin00, dest00, origin01, dest01,
    // origin10, dest10, origin11, dest11 (main.cpp:355-358); nullptr: the default view.
    std::vector<unsigned char> render(const Vec3Df *corners = nullptr, uint64_t rays[3] = nullptr) {
        rt_params p = params();
        if (corners) {
            for (int i = 0; i < 8; ++i)
                for (int k = 0; k < 3; ++k) p.corners[i][k] = corners[i][k];
        } else {
            check(rt_default_corners(p.width, p.height, p.corners));
        }
        std::vector<unsigned char> img(3u * WindowSize_X * WindowSize_Y);
        check(rt_render_tile(scene_, &p, 0, 0, p.width, p.height, img.data(), nullptr, rays));
        return img;
    }

    // Image::writeImage (main.cpp:106-128)
    void writeImage(const char *filename, const std::vector<unsigned char> &rgb) const {
        check(rt_write_ppm(filename, static_cast<int32_t>(WindowSize_X), static_cast<int32_t>(WindowSize_Y), rgb.data()));
    }

    rt_scene *scene() const { return scene_; }

    rt_params params() const {
        rt_params p{};
        p.width = static_cast<int32_t>(WindowSize_X);
        p.height = static_cast<int32_t>(WindowSize_Y);
        p.pfx = static_cast<int32_t>(pixelfactorX);
        p.pfy = static_cast<int32_t>(pixelfactorY);
        p.max_lvl = max_lvl;
        p.flags = (Ambient ? RT_AMBIENT : 0u) | (Diffuse ? RT_DIFFUSE : 0u) | (Specular ? RT_SPECULAR : 0u) |
                  (Reflection ? RT_REFLECTION : 0u) | (Shadows ? RT_SHADOWS : 0u) | (Refraction ? RT_REFRACTION : 0u);
        // any number of lights (the reference's list is an unbounded vector): the first RT_MAX_LIGHTS
        // inline, and the whole list through light_list (Vec3Df is three packed floats), read during the call
        p.n_lights = static_cast<int32_t>(MyLightPositions.size());
        for (size_t i = 0; i < MyLightPositions.size() && i < RT_MAX_LIGHTS; ++i)
            for (int k = 0; k < 3; ++k) p.lights[i][k] = MyLightPositions[i][k];
        if (MyLightPositions.size() > RT_MAX_LIGHTS) p.light_list = MyLightPositions[0].p;
        for (int k = 0; k < 3; ++k) p.camera_pos[k] = MyCameraPosition[k];
        return p;
    }

  private:
    int device_;
    rt_scene *scene_ = nullptr;
};

}  // namespace rtamd

#endif  // RAYTRACERT_HPP_
