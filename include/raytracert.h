/*
 * raytracert.h — C-ABI of librtamd.so, the MI355X (gfx950) drop-in for the render path of
 * wmorssink/raytracert (CG_Project). Plain pointers and sizes only; no HIP or torch types.
 *
 * Reference interface each entry replaces (paths relative to the reference's CG_Project/):
 *   rt_scene_load_obj     init(char*)                       raytracing.h:19, raytracing.cpp:42-73
 *                         Mesh::loadMesh / Mesh::loadMtl    mesh.h:176-177, mesh.cpp:95-460
 *                         calculateNormals()                raytracing.h:41, raytracing.cpp:78-86
 *   rt_scene_reserve      the rest of init()'s set-up: buffers for the first frame (raytracing.cpp:42-73)
 *   rt_scene_create       Mesh(vertices, triangles) ctor    mesh.h:175 (+ materials, mesh.h:197-200)
 *   rt_scene_destroy      (globals live for the process: main.cpp:17-18,130)
 *   rt_scene_export       read access to MyMesh / normals   raytracing.h:8, raytracing.cpp:33
 *   rt_scene_set_mesh     (nothing in the reference: the mesh is fixed after init; an extension, as
 *                         rt_scene_update_vertices: vertices, triangles and their materials replaced)
 *   rt_get_material       Material getMaterial(int)         raytracing.h:27, raytracing.cpp:373-376
 *   rt_ray_intersect_triangle  rayIntersectTriangle (batched pairs)  raytracing.cpp:99-154
 *   rt_intersect_mesh     intersectMesh (batched)           raytracing.cpp:161-192
 *   rt_trace_rays         Vec3Df performRayTracing(o, d)    raytracing.h:33, raytracing.cpp:410-416
 *   rt_intersect_mesh_device  intersectMesh, rays and results in device memory   raytracing.cpp:161-192
 *   rt_occluded_device    isShadow's verdict for given rays, in device memory  raytracing.cpp:249-258
 *   rt_trace_rays_device  performRayTracing, rays and colours in device memory raytracing.cpp:410-416
 *   rt_closest_hit_range_device  (an extension: the closest hit within a per-ray distance range, with its
 *                         distance and the reference's s, t; raytracing.cpp:106-149, :182)
 *   rt_occluded_range_device  (an extension: occlusion within a range, isShadow's rule or any opaque triangle)
 *   rt_multi_hit_range_device  (an extension: the first k hits of each ray within a range, from one walk)
 *   rt_closest_point_device  (an extension: the nearest point of the mesh to each query point)
 *   rt_nearest_triangles_device / rt_within_radius_device  (extensions: the k nearest triangles of each query
 *                         point, and whether it has one inside its radius)
 *   rt_point_inside_device / rt_signed_distance_device  (extensions: whether each query point is inside the
 *                         mesh, by crossing parity along an axis, and the closest-point record with that sign)
 *   rt_box_overlap_device / rt_box_occupied_device  (extensions: the triangles that meet each axis-aligned query
 *                         box, lowest indices first, and whether any does)
 *   rt_triangle_overlap_device / rt_triangle_collides_device  (extensions: the triangles that meet each query
 *                         triangle, lowest indices first, and whether any does; with a self index, the scene's
 *                         own self-intersections)
 *   rt_triangle_distance_device / rt_triangle_within_device  (extensions: the scene triangle nearest to each query
 *                         triangle with both witness points, and whether one is within a radius)
 *   rt_debug_trace       debug key 'd' (shoot + trace)     raytracing.cpp:493-510
 *                         (batched; also trace(o,d,lvl) at lvl 0, raytracing.h:30)
 *   rt_render_tile        the 'r'-key frame loop            main.cpp:340-411 (loop :355-395,
 *                         + RGBValue clamp :24-42 + Image::writeImage quantisation :102-128)
 *   rt_render_tiles_device  same loop, interleaved tile shard into a device buffer (multi-GPU)
 *   rt_render_frame_device  same loop, the whole frame into a device buffer (single GPU)
 *   rt_render_frames_device  the loop for several views in one launch (consecutive 'r' presses)
 *   rt_render_frames_sharded  the same loop over N GPUs     (nothing in the reference: SURVEY.md §8e)
 *   rt_comm_*             RCCL communicator for it          (one process or host thread per GPU)
 *   rt_default_corners    produceRay for the 4 corners      main.cpp:300-325,355-358 (+ reshape :288-296)
 *   rt_write_ppm          Image::writeImage                 main.cpp:102-128
 *   rt_ppm_writer_*       the same file, kept mapped for a frame per 'r' press    main.cpp:405
 *
 * Errors: the reference has none (loadMesh returns true always, mesh.cpp:330; a missing OBJ
 * crashes at fclose(NULL), mesh.cpp:329). Here every entry returns RT_OK (0) or a negative
 * RT_E_* code, and rt_last_error_string() describes the last failure on the calling thread.
 */
#ifndef RAYTRACERT_H
#define RAYTRACERT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK        0
#define RT_E_IO     -1   /* OBJ cannot be opened / PPM cannot be written */
#define RT_E_PARSE  -2   /* malformed input the reference would read out of bounds */
#define RT_E_HIP    -3   /* a HIP runtime call or kernel launch failed */
#define RT_E_ARG    -4   /* invalid argument (NULL, negative size, bad tile, too many lights) */
#define RT_E_NOMEM  -5
#define RT_E_NODEV  -6   /* no usable gfx950 device */
#define RT_E_RCCL   -7   /* an RCCL call failed, or the communicator reported an asynchronous error */

/* Lights held inline in rt_params (the reference's MyLightPositions is an unbounded std::vector,
 * raytracing.h:9, grown by the 'L' key, main.cpp:334-336): up to RT_MAX_LIGHTS in lights[][], any
 * number (up to RT_LIGHTS_LIMIT) through rt_params.light_list. */
#define RT_MAX_LIGHTS 16
#define RT_LIGHTS_LIMIT 65536

/* Feature switches (raytracing.cpp:15-20; keyboard keys 1-6, raytracing.cpp:456-473). */
#define RT_AMBIENT    (1u << 0)
#define RT_DIFFUSE    (1u << 1)
#define RT_SPECULAR   (1u << 2)
#define RT_REFLECTION (1u << 3)
#define RT_SHADOWS    (1u << 4)
#define RT_REFRACTION (1u << 5)
#define RT_ALL_FEATURES 0x3Fu
/* Extension (the reference has only the regular pf x pf grid): each sub-sample
 * is jittered inside its grid cell by a counter-based hash of (pixel, sub-sample, seed), so a
 * stochastic frame is still a pure function of its parameters and the CPU restatement checks it
 * bit for bit. Sub-sample (subx, suby) of pixel (x, y): key = (y*width + x)*pfx*pfy + subx*pfy +
 * suby; h1 = fmix32(key ^ fmix32(seed)), h2 = fmix32(h1 + 0x9E3779B9) (MurmurHash3 finaliser);
 * jx = (h1 >> 8) * 2^-24, jy = (h2 >> 8) * 2^-24; xscale = 1 - (x*pfx + (subx + jx)) / divX and
 * likewise y, every operation in binary32. */
#define RT_STOCHASTIC (1u << 8)
#define RT_DEFAULT_SEED 0x5EED

/* Material "is set" flags (mesh.h:116-122). */
#define RT_HAS_KD    (1u << 0)
#define RT_HAS_KA    (1u << 1)
#define RT_HAS_KS    (1u << 2)
#define RT_HAS_NS    (1u << 3)
#define RT_HAS_NI    (1u << 4)
#define RT_HAS_TR    (1u << 5)
#define RT_HAS_ILLUM (1u << 6)

/* Layout-compatible with Vec3Df (Vec3D.h:272,291: float p[3], 12 bytes). */
typedef struct { float x, y, z; } rt_vec3;

/* Material (mesh.h:10-125) as plain data. Values of never-set fields are defined as 0. */
typedef struct {
    float Kd[3], Ka[3], Ks[3];
    float Ns, Ni, Tr;
    int32_t illum;
    uint32_t flags;      /* RT_HAS_* */
} rt_material;

/* Everything the reference reads from globals during a render. */
typedef struct {
    int32_t width, height;        /* WindowSize_X / WindowSize_Y (main.cpp:137-138) */
    int32_t pfx, pfy;             /* pixelfactorX / pixelfactorY (raytracing.cpp:23-25), >= 1 */
    int32_t max_lvl;              /* max recursion level (raytracing.cpp:29), >= 0 */
    uint32_t flags;               /* RT_AMBIENT ... RT_REFRACTION */
    int32_t n_lights;             /* MyLightPositions.size(): 0..RT_MAX_LIGHTS, or 0..RT_LIGHTS_LIMIT with light_list */
    int32_t seed;                 /* RT_STOCHASTIC only (else ignored): jitter hash seed */
    float lights[RT_MAX_LIGHTS][3];
    float camera_pos[3];          /* MyCameraPosition (raytracing.h:10) */
    float corners[8][3];          /* origin00,dest00, origin01,dest01, origin10,dest10, origin11,dest11 */
    /* NULL: the lights are lights[0..n_lights). Else n_lights x 3 floats (host memory, read during the
     * call; a std::vector<Vec3Df>'s data() is such an array) and lights[][] is ignored: any number of
     * lights, shaded in order as shade() loops over MyLightPositions (raytracing.cpp:342). */
    const float *light_list;
} rt_params;

typedef struct rt_scene rt_scene;

/* Pass as `device` to load/create a scene on the host only (loader and inspection; no HIP calls).
 * Render/intersect entries on such a scene return RT_E_NODEV. */
#define RT_HOST_ONLY (-1)

const char *rt_last_error_string(void);
/* Number of visible HIP devices. */
int rt_device_count(int32_t *count);

/* ---- scene ---------------------------------------------------------------------------- */
int  rt_scene_load_obj(const char *path, int32_t device, rt_scene **out);
/* load_flags: RT_LOAD_PARALLEL (what rt_scene_load_obj does: the file is parsed by up to 16
 * threads) or RT_LOAD_SEQUENTIAL (one fgets/sscanf pass, the reference loader restated line by
 * line). Both produce the same vertices, triangles, materials and normals bit for bit. */
#define RT_LOAD_PARALLEL   0
#define RT_LOAD_SEQUENTIAL 1
#define RT_LOAD_THREADS(n) ((n) << 8)   /* with RT_LOAD_PARALLEL: exactly n parser threads (tests) */
/* | RT_LOAD_TEXCOORDS: also keep Mesh::texcoords and Triangle::t (mesh.cpp:199-209, 263-268,
 * 290-316; the sequential parse), read back with rt_scene_texcoords. The tracer never uses them. */
#define RT_LOAD_TEXCOORDS  0x10
int  rt_scene_load_obj_ex(const char *path, int32_t device, int32_t load_flags, rt_scene **out);
/* Texture coordinates of a scene loaded with RT_LOAD_TEXCOORDS: *n_texcoords `vt` entries as 3
 * floats each (x, y, 0: the reference reads 2D coordinates into a Vec3Df), and per triangle its
 * three texture-coordinate indices (Triangle::t: the face's 1-based indices minus 1, as unsigned;
 * 0 for corners without one, mesh.cpp:290-291). Any pointer may be NULL; sizes 3*n, 3*nt. */
int  rt_scene_texcoords(const rt_scene *scene, int32_t *n_texcoords, float *texcoords, uint32_t *tri_t);
/* Mesh::loadMtl's parse (mesh.cpp:334-460) of one MTL file: every block the reference would
 * commit, in file order (unset values inherited from the previous block, `d` and `Tr` both set
 * Tr). Mesh::loadMtl then appends each block whose name is not yet in its materialIndex (the
 * first of a name wins). *n_blocks = the count; materials (capacity entries, may be NULL) and
 * names (NUL-separated, may be NULL; names_capacity must hold them all) receive them.
 * RT_E_IO if the file cannot be opened (the reference prints a warning and returns false). */
int  rt_load_mtl(const char *path, int32_t *n_blocks, rt_material *materials, int32_t capacity, char *names,
                 size_t names_capacity);
int  rt_scene_create(const float *xyz, int32_t n_vertices, const uint32_t *tri_v, const uint32_t *tri_mat,
                     int32_t n_triangles, const rt_material *materials, int32_t n_materials,
                     int32_t device, rt_scene **out);
void rt_scene_destroy(rt_scene *scene);
int  rt_scene_info(const rt_scene *scene, int32_t *n_vertices, int32_t *n_triangles, int32_t *n_materials);
/* Host copies of the loaded scene; any pointer may be NULL. Sizes: 3*nv, 3*nt, nt, nm, 3*nt.
 * face_normals of a device scene are the ones its renderer uses, computed on the device at upload
 * (calculateNormals, raytracing.cpp:78-86); of a host-only scene, the loader's (bit-identical). */
int  rt_scene_export(const rt_scene *scene, float *vertices, uint32_t *tri_v, uint32_t *tri_mat,
                     rt_material *materials, float *face_normals);
int  rt_get_material(const rt_scene *scene, int32_t triangle_index, rt_material *out);
/* Dynamic geometry (an extension: the reference's mesh is fixed after init, raytracing.cpp:42-76). New
 * positions for the scene's vertices, xyz = 3 * n_vertices floats with n_vertices the scene's own count;
 * triangles, materials and texture coordinates stay. After a successful return every entry behaves bit
 * for bit as on a scene created from the same arrays: intersectMesh's result is the (distance, index)
 * minimum over accepted triangles (raytracing.cpp:161-192) whatever the tree's shape, so the BVH keeps
 * its topology and only its boxes are recomputed (a refit; on a device scene by HIP kernels from a
 * persistent device copy of the vertices). The trees are rebuilt from the new vertices when some
 * triangle moved between the classes the topology bakes in (in the tree / ill-conditioned and tested by
 * every query / degenerate and never accepted), or on request (RT_UPDATE_REBUILD: a refitted tree of a
 * heavily deformed mesh renders the same bytes more slowly). *outcome (may be NULL) says which happened.
 * The update runs after every render queued on the scene before it and is complete on return. Batch
 * orders, launch trials and workspaces are kept. RT_E_ARG (scene untouched) for a NULL scene or array, a
 * wrong vertex count or an unknown mode. */
#define RT_UPDATE_AUTO      0   /* refit; rebuild only if some triangle changed class */
#define RT_UPDATE_REBUILD   1   /* always rebuild the trees from the new vertices */
#define RT_UPDATED_REFIT    0
#define RT_UPDATED_REBUILT  1
int  rt_scene_update_vertices(rt_scene *scene, const float *xyz, int32_t n_vertices, int32_t mode, int32_t *outcome);
/* The same from device memory on the scene's device (e.g. a simulation's output; no host copy unless
 * the trees are rebuilt). The array must be complete when the call is made: it is read on the scene's
 * own stream. RT_E_NODEV on a host-only scene. */
int  rt_scene_update_vertices_device(rt_scene *scene, const void *d_xyz, int32_t n_vertices, int32_t mode,
                                     int32_t *outcome);
/* Topology changes (an extension; nothing in the reference, whose mesh is fixed after init): replace the
 * scene's vertices, triangle indices and triangle materials. The counts may differ from the scene's in
 * either direction, n_triangles == 0 included. The material table, the chosen builder, the accel mode, the
 * profiling mode and the tuning knobs stay; texture coordinates are dropped (rt_scene_texcoords then
 * reports 0 texcoords and a zero tri_t). After a successful return every entry behaves bit for bit as on a
 * scene made by rt_scene_create_ex from the same arrays, the scene's materials and the scene's builder
 * (frames, host and device queries, rt_debug_trace, rt_scene_export, rt_get_material, rt_scene_bvh_*, a
 * later rt_scene_update_vertices). *outcome (may be NULL) reports the builder that made the new trees with
 * the RT_UPDATED_REBUILT* values, as an update does (RT_MESH_REPLACED names the call's plain success).
 * The work runs on the scene's stream after every render and device query queued before it and is complete
 * on return: a query queued before answers for the old mesh, one queued after for the new. Render
 * workspaces, streams, events, the stack overflow area and the builders' scratch are kept; batch orders
 * and launch trials are reset to a new scene's; per-triangle and per-vertex device buffers are reallocated
 * only when a count exceeds their capacity (with a device builder a replacement inside it allocates
 * nothing). On a host-only scene rt_scene_set_mesh runs creation's host path.
 * Errors, the scene untouched and still answering for the old mesh: RT_E_ARG for a NULL scene, a negative
 * count, a NULL array with a non-zero count; RT_E_PARSE "triangle references a missing vertex" /
 * "triangle references a missing material" (rt_scene_create_ex's checks and texts). */
#define RT_MESH_REPLACED 0
int  rt_scene_set_mesh(rt_scene *scene, const float *xyz, int32_t n_vertices, const uint32_t *tri_v,
                       const uint32_t *tri_mat, int32_t n_triangles, int32_t *outcome);
/* The same from device memory on the scene's device, complete when the call is made (read on the scene's
 * own stream). With RT_BUILD_LBVH / RT_BUILD_CLUSTER nothing is copied to the host: the indices are
 * validated by a kernel whose verdict is read before anything dereferences one, records, normals and
 * trees are made by the kernels of rt_scene_update_vertices and of the builders, and the host mirror is
 * read back only when a host consumer asks. d_counts (may be NULL): a device int32[2] {live vertices,
 * live triangles}, read in stream order (one 8-byte synchronising read) and clamped to [0, n_vertices] /
 * [0, n_triangles], which are then the arrays' capacities; entries past the live counts are never read and
 * the scene afterwards has the live counts (rt_scene_info). RT_E_NODEV on a host-only scene (checked
 * first); RT_E_ARG also for a device pointer that is not 4-byte aligned. */
int  rt_scene_set_mesh_device(rt_scene *scene, const void *d_xyz, int32_t n_vertices, const void *d_tri_v,
                              const void *d_tri_mat, int32_t n_triangles, const void *d_counts, int32_t *outcome);

/* ---- tree builder ---------------------------------------------------------------------
 * Which builder makes a scene's trees. Every builder gives the same output bytes (any tree whose boxes
 * contain the padded acceptance boxes below them does); they differ in build time and frame time.
 * RT_BUILD_SAH, the default, is the host's binned-SAH build. RT_BUILD_LBVH is a Morton-order radix tree
 * (Karras 2012): on a device scene it is built by HIP kernels from the device-resident vertices, with
 * no host build and no upload; on a host-only scene the same tree is built on the CPU. A tree that
 * would break a limit of the traversal (more than 40 levels, the leaf index field, boxes that cannot
 * be quantised) is built by the SAH builder instead, without an error.
 * RT_BUILD_CLUSTER is an agglomerative builder (parallel locally-ordered clustering, Meister & Bittner
 * 2018): it keeps the Morton builder's leaf order and replaces the radix tree by nearest-neighbour merges
 * on the surface area of the union box, so that a few huge triangles no longer inflate the upper boxes.
 * On a device scene HIP kernels build it from the device-resident vertices, on a host-only scene the CPU
 * builds the same arrays bit for bit. A tree that would break a limit (depth, leaf index field, boxes that
 * cannot be quantised), or a clustering that does not finish within its iteration budget, is built by
 * the Morton builder instead (which keeps its own fallback to SAH), without an error: built_with and the
 * update's outcome report the builder that made the trees (rt_scene_build_info reports why).
 * rt_scene_set_builder rebuilds nothing: it chooses the builder of the scene's later builds
 * (RT_UPDATE_REBUILD, RT_UPDATE_AUTO's rebuild after a class change, a lazy first build). RT_E_ARG
 * (scene untouched) for an unknown value. rt_scene_get_builder reports the chosen builder and the one
 * that built the trees the scene holds now (either pointer may be NULL).
 * *outcome of rt_scene_update_vertices[_device] is RT_UPDATED_REBUILT_LBVH when the Morton-order
 * builder made the new trees and RT_UPDATED_REBUILT_CLUSTER when the agglomerative one did;
 * RT_UPDATED_REBUILT keeps meaning the host SAH build.
 * rt_scene_create_ex is rt_scene_create with the builder of the scene's first trees. */
#define RT_BUILD_SAH   0
#define RT_BUILD_LBVH  1
#define RT_BUILD_CLUSTER 2
#define RT_UPDATED_REBUILT_LBVH 2
#define RT_UPDATED_REBUILT_CLUSTER 3
int  rt_scene_set_builder(rt_scene *scene, int32_t builder);
int  rt_scene_get_builder(const rt_scene *scene, int32_t *selected, int32_t *built_with);
int  rt_scene_create_ex(const float *xyz, int32_t n_vertices, const uint32_t *tri_v, const uint32_t *tri_mat,
                        int32_t n_triangles, const rt_material *materials, int32_t n_materials,
                        int32_t device, int32_t builder, rt_scene **out);

/* ---- hot path ------------------------------------------------------------------------- */
/* rayIntersectTriangle (raytracing.cpp:99-154) for n independent (ray, triangle) pairs on device
 * `device`: rays = n x {origin, dest} (6 floats), tris = n x {T0, T1, T2} (9 floats), host arrays.
 * hit[i] = 1 and points[3*i..] = the intersection point (the reference's intersectOut), or 0 and
 * (0,0,0). No distance compare: a hit whose point is not finite is reported as the reference does. */
int rt_ray_intersect_triangle(int32_t device, const float *rays, const float *tris, int32_t n, uint8_t *hit,
                              float *points);
/* Batched intersectMesh: n rays (origin[i], dest[i], host arrays of 3*n floats).
 * index_out[i] = closest triangle or -1; point_out[3*i..] = hit point or (0,0,0).
 * Any float32 rays, here and in every ray entry below: the answer is the reference's bit for bit (no hit for a NaN
 * or infinite component); only speed depends on the ray (|dest - origin| outside [2^-63, 2^63] walks without the
 * distance cull, a ray long enough for n.dir to overflow meets every triangle). */
int rt_intersect_mesh(rt_scene *scene, const float *origins, const float *dests, int32_t n,
                      int32_t *index_out, float *point_out);
/* Batched performRayTracing: rgb_out[3*i..] = unclamped colour of ray i.
 * counts (may be NULL) receives {primary, secondary, shadow} intersectMesh-equivalent queries. */
int rt_trace_rays(rt_scene *scene, const rt_params *params, const float *origins, const float *dests,
                  int32_t n, float *rgb_out, uint64_t counts[3]);

/* Device-resident ray queries (extensions: the reference's rays live in host Vec3Df's). The three entries
 * below answer n rays that are already in DEVICE memory on the scene's device and write their results to
 * DEVICE memory, on the caller's stream: no host copy and, unless stated, no host synchronisation. Ray i is
 * the half-line from origin[i] through dest[i], exactly as the host entries read it. ray_stride says how the
 * two ray arrays are laid out: RT_RAYS_PACKED, a contiguous float32 (n,3) array; RT_RAYS_PADDED, (n,4) with
 * w ignored and the array 16-byte aligned. Results are always packed. Outputs must not overlap inputs
 * (nor d_count): the kernels read the rays while they write results.
 * stream is the caller's hipStream_t (NULL = the null stream), semantics as rt_render_tiles_device: the work
 * starts after what is already queued on the stream and later work queued on it sees the results.
 * A later rt_scene_update_vertices[_device], tree rebuild or rt_scene_destroy waits for the queries still in
 * flight before it writes or frees what they read, so a query queued before an update answers for the old
 * vertices and one queued after it for the new.
 * d_count (rt_intersect_mesh_device, rt_occluded_device; may be NULL): a device int32 that the kernel reads
 * when it runs, in stream order, never on the host; the live ray count is min(max(*d_count, 0), n), n is then
 * the capacity the launch is sized for, and output elements at or past the live count are not written. A
 * producer kernel on the same stream can thus decide the count without a host synchronisation.
 * Errors (scene untouched, nothing enqueued): RT_E_NODEV on a host-only scene (checked first); RT_E_ARG for a
 * NULL scene, n < 0, a ray_stride other than 3 or 4, a NULL array with n > 0, a pointer that is not 4-byte
 * aligned (16-byte for the ray arrays at RT_RAYS_PADDED). n == 0 is RT_OK with nothing enqueued. */
#define RT_RAYS_PACKED 3   /* x,y,z per ray, 12 bytes apart: a contiguous float32 (n,3) array */
#define RT_RAYS_PADDED 4   /* x,y,z,w per ray, 16 bytes apart, w ignored; 16-byte aligned */
/* intersectMesh (raytracing.cpp:161-192) for rays in device memory: d_index_out[i] (n x int32) = closest
 * triangle or -1, d_point_out[3*i..] (3n packed floats) = hit point or (0,0,0), bit for bit what
 * rt_intersect_mesh returns for the same rays. Returns after enqueueing; uses no render workspace. */
int rt_intersect_mesh_device(rt_scene *scene, const void *d_origins, const void *d_dests, int32_t ray_stride,
                             int32_t n, const void *d_count, void *d_index_out, void *d_point_out, void *stream);
/* isShadow's verdict (raytracing.cpp:249-258) for caller-given rays: d_blocked_out[i] (n x uint8) = 1 when
 * the ray's CLOSEST hit exists and its material is not transparent (transparent: RT_HAS_TR and Tr < 1,
 * raytracing.cpp:254), else 0. As in the reference a transparent closest hit does not block whatever lies
 * behind it. No 0.1 offset is added (raytracing.cpp:246 is the frame path's own): the caller supplies the
 * origin it wants. Returns after enqueueing; uses no render workspace. */
int rt_occluded_device(rt_scene *scene, const void *d_origins, const void *d_dests, int32_t ray_stride,
                       int32_t n, const void *d_count, void *d_blocked_out, void *stream);
/* Ranged device queries (extensions): the two queries above restricted to a per-ray distance range, with a
 * hit record in place of the bare index. Everything is decided in binary32.
 * A triangle is ACCEPTED by ray i exactly when rayIntersectTriangle accepts it (raytracing.cpp:106-149), and
 * its distance is the float intersectMesh compares (:182). It is IN RANGE iff tmin_i <= distance < tmax_i, with
 *   tmin_i = d_tmin ? d_tmin[i] : 0
 *   tmax_i = d_tmax ? d_tmax[i] : (flags & RT_RANGE_TO_DEST) ? |dest - origin| : +inf
 * (|dest - origin| = sqrtf((dx*dx + dy*dy) + dz*dz), the reference's Vec3D length), both clamped above to
 * FLT_MAX as intersectMesh's own bound is. With d_tmax given RT_RANGE_TO_DEST has no effect. A NaN bound,
 * tmax <= 0 or tmin >= tmax is an empty range: a miss. d_tmin / d_tmax are n device floats each (4-byte
 * aligned) or NULL; rows at or past the live count are not read.
 * Rays, ray_stride, d_count, stream, ordering against updates, and the errors are those of the entries above;
 * in addition RT_E_ARG for d_hit_out not 16-byte aligned, d_tmin / d_tmax not 4-byte aligned, an unknown
 * flag bit, or a flag the entry does not use. Outputs must not overlap the rays, the bounds or d_count. */
typedef struct {
    int32_t triangle;   /* the closest in-range accepted triangle, or -1 */
    float distance;     /* its distance (raytracing.cpp:182), +inf on a miss */
    float s, t;         /* the reference's parametric coordinates of the hit (:144, :148): the point is
                           V0 + s (V1 - V0) + t (V2 - V0); 0, 0 on a miss */
} rt_hit;               /* 16 bytes */
#define RT_RANGE_TO_DEST      (1u << 0)   /* tmax defaults to the ray's own length: the segment origin..dest */
#define RT_OCCLUDE_ANY_OPAQUE (1u << 1)   /* rt_occluded_range_device: any non-transparent triangle in range blocks */
/* d_hit_out[i] (n x rt_hit, 16-byte aligned) = the lexicographic (distance, index) minimum over the in-range
 * accepted triangles, or {-1, +inf, 0, 0}; d_point_out (3n packed floats, may be NULL) = the intersection
 * point (:130) or (0,0,0). With both bounds NULL and flags 0, triangle and point are rt_intersect_mesh_device's
 * bits. tmin = nextafterf(previous distance, +inf) steps to the next distance along the ray; it skips every
 * other accepted triangle at the previous distance (duplicated or coincident geometry, shared edges), which
 * rt_multi_hit_range_device does not.
 * flags: RT_RANGE_TO_DEST. */
int rt_closest_hit_range_device(rt_scene *scene, const void *d_origins, const void *d_dests, int32_t ray_stride,
                                int32_t n, const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags,
                                void *d_hit_out, void *d_point_out, void *stream);
/* d_blocked_out[i] (n x uint8): by default isShadow's rule inside the range, 1 when the closest in-range
 * accepted triangle exists and its material is not transparent; with RT_OCCLUDE_ANY_OPAQUE, 1 when SOME
 * in-range accepted triangle's material is not transparent (line of sight: glass in front of a wall does not
 * hide the wall). With RT_RANGE_TO_DEST this answers "are origin and dest mutually visible".
 * flags: RT_RANGE_TO_DEST, RT_OCCLUDE_ANY_OPAQUE. */
int rt_occluded_range_device(rt_scene *scene, const void *d_origins, const void *d_dests, int32_t ray_stride,
                             int32_t n, const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags,
                             void *d_blocked_out, void *stream);
/* The first k hits of each ray, from one walk. Accepted, distance, in range, the bounds, RT_RANGE_TO_DEST, the
 * FLT_MAX clamp, empty ranges, rays, ray_stride, d_count, stream and the ordering against updates, rebuilds,
 * rt_scene_set_mesh and rt_scene_destroy are exactly those of rt_closest_hit_range_device.
 * d_hits_out (n x k rt_hit, ray-major, 16-byte aligned): with m the number of in-range accepted triangles of
 * ray i, rows [i*k, i*k + min(m, k)) are those triangles' records in ascending lexicographic (distance, index)
 * order, each with the distance, s, t bits rt_closest_hit_range_device gives for that triangle; the ray's
 * other rows are the miss record {-1, +inf, 0, 0}. Triangles at one distance all appear, lowest index first:
 * nothing is skipped as stepping by nextafterf does. With k = 1 and no flag, row i is
 * rt_closest_hit_range_device's record bit for bit.
 * d_nhits_out (n x int32, 4-byte aligned; may be NULL unless RT_MULTI_COUNT_ALL): min(m, k), or with
 * RT_MULTI_COUNT_ALL m itself (so a caller sees that k truncated the list, or reads the crossing parity with
 * k = 1); the hit rows are the same bytes either way. Rays at or past the live count are not written.
 * flags: RT_RANGE_TO_DEST, RT_MULTI_COUNT_ALL. Errors as the ranged entries; in addition RT_E_ARG for k < 1 or
 * k > RT_MULTI_HIT_MAX, d_hits_out NULL (n > 0) or not 16-byte aligned, d_nhits_out not 4-byte aligned,
 * RT_MULTI_COUNT_ALL with a NULL d_nhits_out, n * k above INT32_MAX. */
#define RT_MULTI_HIT_MAX   16
#define RT_MULTI_COUNT_ALL (1u << 2)      /* d_nhits_out = all in-range accepted triangles, not min(m, k) */
int rt_multi_hit_range_device(rt_scene *scene, const void *d_origins, const void *d_dests, int32_t ray_stride,
                              int32_t n, const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags,
                              int32_t k, void *d_hits_out, void *d_nhits_out, void *stream);
/* The nearest point of the mesh to each query point (an extension: no ray is involved).
 * d_points: n points, float32 in device memory on the scene's device, point_stride RT_RAYS_PACKED or
 * RT_RAYS_PADDED (w ignored, 16-byte aligned). d_count, stream and the ordering against updates, rebuilds,
 * rt_scene_set_mesh and rt_scene_destroy are exactly those of rt_closest_hit_range_device; rows at or past the
 * live count are neither read nor written.
 * d_hit_out (n x rt_hit, 16-byte aligned): {triangle, distance, s, t} with the closest point
 * V0 + s (V1 - V0) + t (V2 - V0); a miss is {-1, +inf, 0, 0}. d_point_out (3n packed floats, may be NULL): the
 * closest point c below, or (0,0,0) on a miss. d_rmax (n floats, 4-byte aligned, may be NULL): a search radius
 * per point. flags must be 0 (RT_E_ARG otherwise). Errors as the ranged entries, in their order.
 *
 * The definition. Everything is binary32 without contraction, a dot product is (ax bx + ay by) + az bz,
 * division and sqrtf are correctly rounded. With T0 = V0, u = V1 - V0, v = V2 - V0, uu = dot(u, u),
 * uv = dot(u, v), vv = dot(v, v) (the triangle's record), a triangle is a candidate unless its normal u x v is
 * (0,0,0): the class rt_bvh_acceptance_box reports as 2, the triangles no ray entry ever returns. For a
 * candidate and a point p, with w = p - T0:
 *   d1 = dot(u, w)      d2 = dot(v, w)
 *   d3 = d1 - uu        d4 = d2 - uv
 *   d5 = d1 - uv        d6 = d2 - vv
 *   vc = d1 d4 - d3 d2  vb = d5 d2 - d1 d6  va = d3 d6 - d5 d4
 *   the first that holds:
 *     d1 <= 0 && d2 <= 0                        : s = 0, t = 0                     (vertex 0)
 *     d3 >= 0 && d4 <= d3                       : s = 1, t = 0                     (vertex 1)
 *     vc <= 0 && d1 >= 0 && d3 <= 0             : s = d1 / (d1 - d3), t = 0        (edge 0-1)
 *     d6 >= 0 && d5 <= d6                       : s = 0, t = 1                     (vertex 2)
 *     vb <= 0 && d2 >= 0 && d6 <= 0             : s = 0, t = d2 / (d2 - d6)        (edge 0-2)
 *     va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0   : t = (d4 - d3) / ((d4 - d3) + (d5 - d6)), s = 1 - t   (edge 1-2)
 *     otherwise                                 : q = 1 / ((va + vb) + vc), s = vb q, t = vc q, then
 *                                                 if (s < 0) s = 0; if (s > 1) s = 1; m = 1 - s;
 *                                                 if (t < 0) t = 0; if (t > m) t = m            (interior)
 *   c = (T0 + s u) + t v per component     r = p - c     dist2 = dot(r, r)
 * (The interior's four compares keep s, t inside the triangle when va, vb, vc are rounding noise, as they are far
 * from a small triangle; a NaN passes through them unchanged.)
 * The answer for point i is the lexicographic (dist2, triangle index) minimum over the candidates with
 * dist2 < bound_i; bound_i is +inf when d_rmax is NULL, else rmax_i * rmax_i rounded to float when rmax_i > 0; a
 * NaN, zero or negative radius is an empty search, a miss. The record's distance is sqrtf(dist2).
 * Consequences: a NaN in the arithmetic falls through to the interior case and gives a NaN dist2, which never
 * wins; a point with a NaN or infinite component is a miss; so is a point so far away that dist2 overflows.
 * The result does not depend on the acceleration structure: the tree walk returns the bytes of the loop over
 * every triangle. */
int rt_closest_point_device(rt_scene *scene, const void *d_points, int32_t point_stride, int32_t n,
                            const void *d_count, const void *d_rmax, uint32_t flags,
                            void *d_hit_out, void *d_point_out, void *stream);
/* The same for host arrays (points 3n packed floats, rmax n floats or NULL, point_out 3n floats or NULL):
 * copy in, the same launch, copy out, synchronise. The same bits. */
int rt_closest_point(rt_scene *scene, const float *points, int32_t n, const float *rmax,
                     rt_hit *hit_out, float *point_out);
/* The k nearest triangles of each query point, from one walk. The definition adds no arithmetic: candidate, dist2,
 * s, t, c and bound_i are exactly those of rt_closest_point_device above (a NaN or infinite point component and a
 * NaN, zero or negative radius are empty searches; with d_rmax NULL the bound is +inf). Let m be the number of
 * candidates of point i with dist2 < bound_i.
 * d_hits_out (n x k rt_hit, point-major, 16-byte aligned): rows [i k, i k + min(m, k)) are those candidates in
 * ascending lexicographic (dist2, triangle index) order, each {triangle, sqrtf(dist2), s, t} with the bits
 * rt_closest_point_device computes for that triangle and point; the point's other rows are the miss record
 * {-1, +inf, 0, 0}. Triangles at an equal dist2 (a shared vertex or edge) all appear, lowest index first.
 * d_points_out (n x k x 3 packed floats, may be NULL): c of each row's record, or (0,0,0) on a miss row.
 * d_nfound_out (n x int32, 4-byte aligned; may be NULL unless RT_NEAR_COUNT_ALL): min(m, k), or with
 * RT_NEAR_COUNT_ALL m itself (so a caller sees that k truncated the list); the hit rows are the same bytes
 * whether or not the flag is set. k is in [1, RT_MULTI_HIT_MAX]; with k = 1 and no flag, row i and its point are
 * rt_closest_point_device's bytes. The result does not depend on the acceleration structure.
 * d_points, point_stride, d_count, d_rmax, stream, the ordering against updates, rebuilds, rt_scene_set_mesh and
 * rt_scene_destroy, and rows at or past the live count (neither read nor written) as rt_closest_point_device.
 * Errors in that entry's order: RT_E_NODEV on a host-only scene before anything else; RT_E_ARG for a NULL scene,
 * n < 0, a bad stride, NULL or misaligned arrays, k out of range, any flag but RT_NEAR_COUNT_ALL, that flag with a
 * NULL d_nfound_out, n * k above INT32_MAX; n == 0 returns RT_OK with nothing enqueued. */
#define RT_NEAR_COUNT_ALL (1u << 3)   /* d_nfound_out = every candidate inside the bound, not min(m, k) */
int rt_nearest_triangles_device(rt_scene *scene, const void *d_points, int32_t point_stride, int32_t n,
                                const void *d_count, const void *d_rmax, uint32_t flags, int32_t k,
                                void *d_hits_out, void *d_nfound_out, void *d_points_out, void *stream);
/* Whether anything lies within the radius: d_within_out[i] (n x uint8) is 1 when m > 0 and 0 otherwise, that is,
 * 1 exactly when rt_closest_point_device returns a triangle for that point; the walk leaves a point at its first
 * candidate below the bound. flags must be 0 (RT_E_ARG otherwise). Everything else as the entry above. */
int rt_within_radius_device(rt_scene *scene, const void *d_points, int32_t point_stride, int32_t n,
                            const void *d_count, const void *d_rmax, uint32_t flags,
                            void *d_within_out, void *stream);
/* Whether each query point is inside the mesh: the parity of the number of surface crossings of the half line
 * from the point along a coordinate axis. It means something on a closed (watertight) mesh only; on an open mesh
 * the count is still the defined, deterministic number below, and its parity says nothing.
 * d_points, point_stride, d_count, stream, the ordering against updates, rebuilds, rt_scene_set_mesh and
 * rt_scene_destroy, and rows at or past the live count (neither read nor written) as rt_closest_point_device.
 * axis: RT_AXIS_POS_X .. RT_AXIS_NEG_Z (0..5: +x, -x, +y, -y, +z, -z). flags must be 0.
 * d_inside_out (n x uint8): crossings_i & 1. d_crossings_out (n x int32, 4-byte aligned, may be NULL): crossings_i.
 *
 * The definition. The candidates are rt_closest_point_device's: every triangle whose record normal is not
 * (0,0,0), classes 0 and 1 of rt_bvh_acceptance_box; class 2 never counts. V0, V1, V2 are the scene's current
 * vertex array entries xyz[tri_v[3 i + j]] (not T0 + u: a shared vertex has the same bits in every triangle that
 * uses it). With k = axis >> 1, sg = +1 for an even axis and -1 for an odd one, (a, b) = ((k + 1) % 3, (k + 2) % 3):
 * a point with a NaN or infinite component has crossings 0. Otherwise, no contraction anywhere, per candidate:
 *   d_j = V_j - p per component, one binary32 subtraction each                       (j = 0, 1, 2)
 *   X_j = (double)d_j[a]     Y_j = (double)d_j[b]     Z_j = sg * (double)d_j[k]
 *   for the edges (i0, i1) = (1, 2), (2, 0), (0, 1), giving E_0, E_1, E_2 (E_j is the edge opposite vertex j):
 *     E = X_i0 * Y_i1 - Y_i0 * X_i1 in binary64 (both products are exact: 24-bit factors; E has the exact sign)
 *     the edge is crossed when (Y_i0 <= 0 && Y_i1 > 0 && E > 0) || (Y_i1 <= 0 && Y_i0 > 0 && E < 0)
 *   the triangle covers the point when an odd number of its three edges is crossed
 *   det = (E_0 + E_1) + E_2      num = (E_0 * Z_0 + E_1 * Z_1) + E_2 * Z_2      in binary64
 *   the triangle is above when (det > 0 && num > 0) || (det < 0 && num < 0)
 * crossings_i = the number of candidates that both cover point i and are above it; inside_i = crossings_i & 1.
 * Consequences: the cover test is an exact even-odd test on the projected mesh whose vertices are the d_j, so two
 * triangles that share an edge never both claim, or both drop, a point under that edge; a point exactly under an
 * edge (E = 0) is claimed through that edge by neither; a triangle edge-on to the axis never counts. The above test
 * rounds (E * Z), so a point within rounding of the surface lands on either side: the sign is exact away from the
 * surface and arbitrary but deterministic on it. Six directions let a caller vote. Coordinates are assumed small
 * enough that V_j - p does not overflow binary32. The result does not depend on the acceleration structure: the
 * tree walk returns the count of the loop over every triangle, on any builder, either tree width, after any refit.
 * Errors in rt_closest_point_device's order: RT_E_NODEV on a host-only scene before anything else; RT_E_ARG for a
 * NULL scene, n < 0, a bad stride, NULL or misaligned arrays, a non-zero flag, an axis outside 0..5; n == 0 returns
 * RT_OK with nothing enqueued. */
#define RT_AXIS_POS_X 0
#define RT_AXIS_NEG_X 1
#define RT_AXIS_POS_Y 2
#define RT_AXIS_NEG_Y 3
#define RT_AXIS_POS_Z 4
#define RT_AXIS_NEG_Z 5
int rt_point_inside_device(rt_scene *scene, const void *d_points, int32_t point_stride, int32_t n,
                           const void *d_count, int32_t axis, uint32_t flags,
                           void *d_inside_out /* n x uint8 */, void *d_crossings_out /* n x int32, may be NULL */,
                           void *stream);
/* The signed distance: d_hit_out and d_point_out are rt_closest_point_device's bytes for the same points and
 * d_rmax, with the sign bit of `distance` set when inside_i (above, along `axis`) is 1. A miss outside stays
 * {-1, +inf, 0, 0}; a miss inside is {-1, -inf, 0, 0}, so a narrow-band field keeps its sign beyond the band; s, t
 * and the closest point are unchanged; a point with a NaN or infinite component is a positive miss.
 * d_inside_out (n x uint8, may be NULL): inside_i. It is the closest-point launch followed by the inside launch on
 * the same stream. Arguments and errors as rt_closest_point_device, then the axis. */
int rt_signed_distance_device(rt_scene *scene, const void *d_points, int32_t point_stride, int32_t n,
                              const void *d_count, const void *d_rmax, int32_t axis, uint32_t flags,
                              void *d_hit_out, void *d_point_out /* may be NULL */,
                              void *d_inside_out /* may be NULL */, void *stream);
/* The triangles that meet each axis-aligned query box, from one walk. d_lo and d_hi are the boxes' lower and upper
 * corners, laid out as d_origins / d_dests of the ray entries (box_stride RT_RAYS_PACKED or RT_RAYS_PADDED, w
 * ignored). d_count, stream, the ordering against updates, rebuilds, rt_scene_set_mesh and rt_scene_destroy, and rows
 * at or past the live count (neither read nor written) as rt_closest_point_device. k is in [1, RT_MULTI_HIT_MAX].
 * d_after (n x int32, 4-byte aligned, may be NULL): after_i, or -1 for every box when NULL.
 * Let m be the number of candidates of box i that overlap it (below) and whose triangle index is greater than after_i.
 * d_tris_out (n x k int32, box-major, 4-byte aligned): rows [i k, i k + min(m, k)) are the lowest of those indices in
 * ascending order; the box's other rows are -1. d_nfound_out (n x int32, 4-byte aligned; may be NULL unless
 * RT_BOX_COUNT_ALL): min(m, k), or with RT_BOX_COUNT_ALL m itself; the list is the same bytes whether or not the flag
 * is set. A caller pages through a crowded box by passing the last index it received as after_i (the index-order
 * analogue of stepping tmin).
 *
 * The definition. The candidates are rt_closest_point_device's: every triangle whose record normal is not (0,0,0).
 * V_0, V_1, V_2 are the scene's current vertex array entries xyz[tri_v[3 t + j]]. A box with a NaN or infinite
 * component, or with lo_a > hi_a on some axis, is empty: m = 0. lo == hi is a valid point box; a box is closed, so
 * touching is overlap. No contraction anywhere. A candidate overlaps exactly when none of these tests separates it:
 *   1. raw compares, no arithmetic: separated if on some axis a every V_j[a] > hi_a, or every V_j[a] < lo_a
 *      (min_j V_j[a] > hi_a or max_j V_j[a] < lo_a)
 *   2. c = (lo + hi) * 0.5f and h = (hi - lo) * 0.5f per component, v_j = V_j - c per component, all binary32;
 *      from here on everything is binary64: v_j and h widened
 *   3. the edges f_0 = v_1 - v_0, f_1 = v_2 - v_1, f_2 = v_0 - v_2; for each edge f and each axis a, with
 *      (b, c) = ((a + 1) % 3, (a + 2) % 3):
 *        p_j = f[b] * v_j[c] - f[c] * v_j[b]   (j = 0, 1, 2)        r = h[b] * |f[c]| + h[c] * |f[b]|
 *      separated if every p_j > r, or every p_j < -r (min_j p_j > r or max_j p_j < -r)
 *   4. n = f_0 x f_1, n[a] = f_0[b] * f_1[c] - f_0[c] * f_1[b];  d = (n[0] v_0[0] + n[1] v_0[1]) + n[2] v_0[2];
 *      r = (h[0] |n[0]| + h[1] |n[1]|) + h[2] |n[2]|;  separated if d > r or d < -r
 * Consequences: by step 1 an overlapping triangle's own box meets the query box, so a tree walk that skips a child
 * exactly when lo_a > child_hi_a or hi_a < child_lo_a on some axis loses nothing and needs no margin: the result is
 * the list of the loop over every triangle, on any builder, either tree width, after any refit. A NaN produced in
 * steps 2 to 4 separates nothing. Coordinates are assumed small enough that hi - lo and V_j - c do not overflow.
 * The verdict is exact (the closed triangle meets the closed box) wherever the binary32 centring is exact, for
 * example on dyadic coordinates; elsewhere it is bracketed by the box shrunk and grown by 2^-18 of the largest
 * coordinate magnitude, and within that band, at touching, it is deterministic but not guaranteed: a point box on a
 * shared vertex may claim only some of the triangles around it.
 * Errors in rt_nearest_triangles_device's order: RT_E_NODEV on a host-only scene before anything else; RT_E_ARG for a
 * NULL scene, n < 0, a bad stride, NULL or misaligned arrays, k out of range, any flag but RT_BOX_COUNT_ALL, that flag
 * with a NULL d_nfound_out, n * k above INT32_MAX; n == 0 returns RT_OK with nothing enqueued. */
#define RT_BOX_COUNT_ALL (1u << 4)   /* d_nfound_out = every overlapping candidate past `after`, not min(m, k) */
int rt_box_overlap_device(rt_scene *scene, const void *d_lo, const void *d_hi, int32_t box_stride, int32_t n,
                          const void *d_count, const void *d_after /* n x int32, may be NULL */, uint32_t flags, int32_t k,
                          void *d_tris_out /* n x k int32 */, void *d_nfound_out /* n x int32 */, void *stream);
/* Whether anything meets the box: d_occupied_out[i] (n x uint8) is 1 when m > 0 (after_i = -1) and 0 otherwise; the
 * walk leaves a box at its first overlapping candidate. flags must be 0 (RT_E_ARG otherwise). Everything else as the
 * entry above. */
int rt_box_occupied_device(rt_scene *scene, const void *d_lo, const void *d_hi, int32_t box_stride, int32_t n,
                           const void *d_count, uint32_t flags, void *d_occupied_out /* n x uint8 */, void *stream);
/* The triangles that meet each query triangle, from one walk: the narrow phase of mesh against mesh. d_qtris holds
 * 3 n vertices, query-major: vertex 3 i + j is Q_j of query i, laid out as d_origins of the ray entries (tri_stride
 * RT_RAYS_PACKED: 36 bytes per triangle, 4-byte aligned; RT_RAYS_PADDED: three float4 per triangle, 16-byte aligned,
 * w ignored). d_count, stream, the ordering against updates, rebuilds, rt_scene_set_mesh and rt_scene_destroy, rows
 * at or past the live count, k, d_after, d_tris_out (ascending indices, then -1), d_nfound_out (min(m, k), or m with
 * RT_TRI_COUNT_ALL) and paging by after_i are rt_box_overlap_device's, with "query triangle" for "box": m is the number
 * of candidates of query i that overlap it (below), whose index is greater than after_i, and that self_i does not
 * pass over.
 * d_self (n x int32, 4-byte aligned, may be NULL): self_i in [0, nt) names a scene triangle; candidate t is then
 * passed over when t == self_i or when any of tri_v[3 t .. 3 t + 2] equals any of tri_v[3 self_i .. 3 self_i + 2]
 * (index compares, no geometry). Any other value, and a NULL array, passes nothing over. With query i = scene
 * triangle i, self_i = i and after_i = i, the lists are every intersecting pair of triangles without a common
 * vertex index, each pair exactly once (at its lower index). A triangle folded onto its own neighbour is therefore
 * not reported, and neither are duplicated vertices that carry different indices treated as shared.
 *
 * The definition. The candidates are rt_box_overlap_device's: every triangle whose record normal is not (0,0,0).
 * V_j = xyz[tri_v[3 t + j]], the scene's current vertex array entries. No contraction anywhere.
 *   0. a query with a NaN or infinite component is empty: m = 0
 *   1. raw compares, no arithmetic: qlo_a = min_j Q_j[a], qhi_a = max_j Q_j[a]; separated if on some axis a every
 *      V_j[a] > qhi_a, or every V_j[a] < qlo_a
 *   2. from here on everything is binary64: u_j[a] = (double)Q_j[a] - (double)Q_0[a] (so u_0 = 0) and
 *      v_j[a] = (double)V_j[a] - (double)Q_0[a]; there is no binary32 centring
 *   3. the edges e_0 = u_1 - u_0, e_1 = u_2 - u_1, e_2 = u_0 - u_2, and f_0, f_1, f_2 the same on v; x cross y is
 *      [a] = x[b] * y[c] - x[c] * y[b] with (b, c) = ((a + 1) % 3, (a + 2) % 3); n_Q = e_0 cross e_1,
 *      n_V = f_0 cross f_1. A query whose n_Q is exactly (0,0,0) is empty: m = 0 (points and segments have other
 *      entries)
 *   4. seventeen axes w: n_Q, n_V, the nine e_i cross f_j, the three n_Q cross e_i and the three n_V cross f_j (these
 *      six decide coplanar pairs). Per axis p_j = (w[0] u_j[0] + w[1] u_j[1]) + w[2] u_j[2] and q_j the same on v_j
 *      (j = 0, 1, 2); separated if every p_i < every q_j (nine compares joined by &&), or every p_i > every q_j
 * A candidate overlaps exactly when neither step 1 nor any axis separates it. All compares are strict, so touching
 * is overlap, and a NaN separates nothing. The verdict is an OR over the axes: the order in which an implementation
 * evaluates them, and whether it stops at the first that separates, changes nothing.
 * Consequences: as for the box entry, step 1 lets a tree walk skip a child exactly when the query's bounds
 * [qlo, qhi] and the child's box are disjoint on some axis, with no margin: the result is the list of the loop over
 * every triangle, on any builder, either tree width, after any refit. Coordinates are assumed small enough that the
 * differences and products of steps 2 to 4 do not overflow binary64.
 * The verdict is exact (the closed triangles meet) wherever the binary64 products and sums are exact, for example
 * on coordinates that are multiples of 2^-4 within +-3. Elsewhere a verdict that differs from the exact one needs a
 * pair within rounding of touching, about 2^-40 of the largest coordinate magnitude; there it is deterministic but
 * not guaranteed.
 * Errors in rt_box_overlap_device's order: RT_E_NODEV on a host-only scene before anything else; RT_E_ARG for a NULL
 * scene, n < 0, a bad stride, a NULL or misaligned array, k out of range, any flag but RT_TRI_COUNT_ALL, that flag
 * with a NULL d_nfound_out, n * k above INT32_MAX; n == 0 returns RT_OK with nothing enqueued. */
#define RT_TRI_COUNT_ALL (1u << 4)   /* d_nfound_out = every overlapping candidate past `after`, not min(m, k) */
int rt_triangle_overlap_device(rt_scene *scene, const void *d_qtris, int32_t tri_stride, int32_t n,
                               const void *d_count, const void *d_after /* n x int32, may be NULL */,
                               const void *d_self /* n x int32, may be NULL */, uint32_t flags, int32_t k,
                               void *d_tris_out /* n x k int32 */, void *d_nfound_out /* n x int32 */, void *stream);
/* Whether anything meets the query triangle: d_collides_out[i] (n x uint8) is 1 when m > 0 (after_i = -1, self_i as
 * given) and 0 otherwise; the walk leaves a query at its first overlapping candidate. flags must be 0 (RT_E_ARG
 * otherwise). Everything else as the entry above. */
int rt_triangle_collides_device(rt_scene *scene, const void *d_qtris, int32_t tri_stride, int32_t n,
                                const void *d_count, const void *d_self /* may be NULL */, uint32_t flags,
                                void *d_collides_out /* n x uint8 */, void *stream);
/* The scene triangle nearest to each query triangle: the clearance of mesh against mesh, from one walk. d_qtris,
 * tri_stride, d_count, d_self, stream, the ordering against updates, rebuilds, rt_scene_set_mesh and
 * rt_scene_destroy, and rows at or past the live count (neither read nor written) are rt_triangle_overlap_device's.
 * d_rmax (n floats, 4-byte aligned, may be NULL): a search radius per query, as rt_closest_point_device's.
 * d_hit_out (n x rt_hit, 16-byte aligned): {triangle, distance, s, t} with the nearest point of the scene triangle
 * c_V = V_0 + s (V_1 - V_0) + t (V_2 - V_0), as the closest-point record; a miss is {-1, +inf, 0, 0}. d_qpoint_out and
 * d_point_out (3n packed floats each, 4-byte aligned, either may be NULL): the witness points on the query triangle
 * and on the scene triangle, or (0,0,0) on a miss. flags must be 0.
 *
 * The definition. A query is empty (a miss) exactly when rt_triangle_overlap_device's is: a NaN or infinite
 * component, or n_Q exactly (0,0,0) (segments and points as degenerate queries are out of scope: points have
 * rt_closest_point_device). The candidates and the self pass-over are that entry's too: every triangle whose record
 * normal is not (0,0,0), less self_i and every triangle that shares a vertex index with it (index compares, no
 * geometry). V_j = xyz[tri_v[3 t + j]], the vertex array entries, not the records.
 * Everything is binary64 without contraction, on u_j[a] = (double)Q_j[a] - (double)Q_0[a] and
 * v_j[a] = (double)V_j[a] - (double)Q_0[a] (that entry's step 2); dot(x, y) = (x[0] y[0] + x[1] y[1]) + x[2] y[2];
 * division is correctly rounded; clamp01(x): if (x < 0) x = 0; if (x > 1) x = 1 (a NaN stays a NaN).
 *   PT(p; a, b, c), a point against a triangle: ab = b - a, ac = c - a, w = p - a, d1 = dot(ab, w), d2 = dot(ac, w),
 *     uu = dot(ab, ab), uv = dot(ab, ac), vv = dot(ac, ac), then d3 .. d6, vc, vb, va and the seven cases of
 *     rt_closest_point_device in its order and with its compares, interior clamp included, all in binary64; they
 *     give s and t and the point x[k] = (a[k] + s ab[k]) + t ac[k]
 *   SS(p0, p1; r0, r1), two segments: g = p1 - p0, h = r1 - r0, r = p0 - r0, a = dot(g, g), e = dot(h, h),
 *     f = dot(h, r), c = dot(g, r), b = dot(g, h), den = a e - b b;
 *     sq = den != 0 ? clamp01((b f - c e) / den) : 0      (parallel edges, a zero denominator: sq = 0)
 *     tv = (b sq + f) / e
 *     if (tv < 0) { tv = 0; sq = clamp01(-c / a); } else if (tv > 1) { tv = 1; sq = clamp01((b - c) / a); }
 *     x[k] = p0[k] + sq g[k], y[k] = r0[k] + tv h[k]
 * The pair has fifteen feature distances, in this order, each with a witness c_Q on the query, a witness c_V on the
 * candidate and d2 = dot(c_Q - c_V, c_Q - c_V):
 *   features 0, 1, 2 (j = 0, 1, 2): PT(u_j; v_0, v_1, v_2): c_Q = u_j, c_V = x; the record's s, t are PT's
 *   features 3, 4, 5 (j = 0, 1, 2): PT(v_j; u_0, u_1, u_2): c_Q = x, c_V = v_j; the record's (s, t) is (0,0), (1,0), (0,1)
 *   features 6 + 3 i + j (i, j = 0, 1, 2, i outer): SS(u_i, u_(i+1)%3; v_j, v_(j+1)%3): c_Q = x, c_V = y; the record's
 *     (s, t) is (tv, 0) for j = 0, (1 - tv, tv) for j = 1 and (0, 1 - tv) for j = 2 (one binary64 subtraction)
 * The feature minimum: m = +inf, and each feature in order takes over when its d2 < m (the first strictly smallest; a
 * NaN d2 never takes over; if none does, the parameters and both witnesses are 0).
 * dist2 = 0 when the pair overlaps by rt_triangle_overlap_device's definition (its steps 1 to 4, unchanged), else
 * dist2 = m. So dist2 == 0 coincides with that entry's verdict, except for a feature minimum that itself rounds
 * to 0. The witnesses and parameters are the feature minimum's in both cases (for a pair that cuts through, the
 * nearest features, not a common point).
 * bound2_i is +inf when d_rmax is NULL, else (double)rmax_i * (double)rmax_i (exact) when rmax_i > 0; a NaN, zero or
 * negative radius is an empty search, a miss. The answer for query i is the lexicographic (dist2, triangle index)
 * minimum over the candidates with dist2 < bound2_i; a NaN dist2 never wins.
 * The record: triangle; distance = sqrtf((float)dist2), correctly rounded (no binary64 square root anywhere); s, t
 * rounded to float. The points: (float)((double)Q_0[a] + c[a]) of c_Q and of c_V.
 * Consequences: the result does not depend on the acceleration structure: the tree walk returns the bytes of the
 * loop over every triangle, on any builder, either tree width, after any refit, ties by index included (several
 * overlapping candidates are all at 0 and the lowest index wins). Coordinates are assumed small enough that nothing
 * overflows binary64. With M = scene's largest |V|_1 + 2 max_j |Q_j|_1 the computed sqrt(dist2) of a pair that does
 * not overlap is at most 37 * 2^-53 * M below the true distance of the two triangles.
 * Errors in rt_triangle_overlap_device's order: RT_E_NODEV on a host-only scene before anything else; RT_E_ARG for a
 * NULL scene, n < 0, a bad stride, a NULL or misaligned array, any flag; n == 0 returns RT_OK with nothing enqueued. */
int rt_triangle_distance_device(rt_scene *scene, const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count,
                                const void *d_rmax /* n floats, may be NULL */, const void *d_self /* may be NULL */,
                                uint32_t flags /* 0 */, void *d_hit_out /* n x rt_hit */,
                                void *d_qpoint_out /* 3n floats, may be NULL */, void *d_point_out /* 3n floats, may be NULL */,
                                void *stream);
/* Whether a scene triangle is within the radius of the query triangle: d_within_out[i] (n x uint8) is 1 exactly when
 * rt_triangle_distance_device returns a triangle for the same arguments, else 0; the walk leaves a query at its first
 * candidate below the bound. Everything else as the entry above. */
int rt_triangle_within_device(rt_scene *scene, const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count,
                              const void *d_rmax, const void *d_self, uint32_t flags /* 0 */,
                              void *d_within_out /* n x uint8 */, void *stream);
/* performRayTracing (raytracing.cpp:410-416) for rays in device memory: d_rgb_out[3*i..] (3n packed floats),
 * bit for bit rt_trace_rays' rgb_out. counts as in rt_trace_rays; non-NULL synchronises the stream. Uses
 * render pipeline 0's workspace (ordered against the frames that use it): returns after enqueueing when
 * counts == NULL and that workspace is already large enough (rt_scene_reserve, or an earlier call of this
 * size). n * max(n_lights, 1) <= 2^30 and the params rules as rt_trace_rays. No d_count: the chain's queues
 * are sized on the host. */
int rt_trace_rays_device(rt_scene *scene, const rt_params *params, const void *d_origins, const void *d_dests,
                         int32_t ray_stride, int32_t n, void *d_rgb_out, void *stream, uint64_t counts[3]);

/* Single-ray debug trace (the reference's key 'd', raytracing.cpp:493-510, which shoots one ray,
 * keeps (origin, intersection) for drawing and prints the traced colour): one record per trace()
 * call of the ray's chain, in order, with the outcome of each shadow ray its shade() cast. For
 * parity triage: compare against the oracle's ora_debug_trace to find the first bounce that
 * differs. Writes min(n, max_bounces) records; *n_bounces = n; rgb = performRayTracing(o, d). */
typedef struct {
    float origin[3], dest[3];     /* the ray trace() was called with */
    float hit[3];                 /* intersectMesh's point, (0,0,0) on a miss */
    int32_t triangle;             /* intersectMesh's index, -1 on a miss */
    int32_t level;                /* trace()'s lvl argument */
    uint32_t shadowed;            /* bit l: light l's shadow ray was blocked (isShadow true) */
    uint32_t lit;                 /* bit l: light l's shadow ray was traced and not blocked */
} rt_debug_bounce;
int rt_debug_trace(rt_scene *scene, const rt_params *params, const float origin[3], const float dest[3],
                   rt_debug_bounce *bounces, int32_t max_bounces, int32_t *n_bounces, float rgb[3]);
/* The frame loop for pixels [x0,x0+w) x [y0,y0+h) of the params->width x params->height frame.
 * rgb_u8 (w*h*3 bytes, row-major, top row first, as written to result.ppm) and rgb_f32
 * (w*h*3 clamped floats) are host buffers; either may be NULL. */
int rt_render_tile(rt_scene *scene, const rt_params *params, int32_t x0, int32_t y0, int32_t w, int32_t h,
                   uint8_t *rgb_u8, float *rgb_f32, uint64_t counts[3]);
/* Interleaved tile shard for multi-GPU rendering, fully device-resident. The frame is cut into
 * tile_w x tile_h tiles numbered row-major (tiles_x = ceil(width/tile_w), T tiles per frame); a batch
 * of `frames` frames of this view has tile ids g = f*T + t. This call renders ids first,
 * first+stride, first+2*stride, ... below frames*T and writes each as tile_w*tile_h*3 bytes (pixels
 * outside the frame are 0) into the DEVICE buffer d_out_u8 in that order. stream is the caller's
 * hipStream_t (NULL = the null stream): the work starts after what is already queued on it and
 * later work queued on it sees the finished tiles (the renderer forks its pipelines from it and
 * joins them back). The call returns after enqueueing (no host synchronisation) unless
 * counts != NULL. Returns the number of tiles written via n_tiles_out. */
/* Every sub-sample of the 'r' loop (main.cpp:369-388) for the frame params describes, in the loop's call
 * order: record k = ((y * width + x) * pfx + subx) * pfy + suby holds performRayTracing(origin, dest) of the
 * loop's ray for (x, y, subx, suby), unclamped (raytracing.cpp:410-416). layout RT_SAMPLES_RGB: 3 floats
 * per record, the colour; RT_SAMPLES_RAY_RGB: 9 floats, the ray's origin and dest as the device made them
 * (the loop's binary32 expressions, main.cpp:380-386), then the colour. A host that runs the loop unchanged
 * can answer each call from here once it finds the call's ray equal to the record's, bit for bit
 * (include/raytracert_dropin.hpp does). out is host memory of `capacity` floats (>= layout x width x height
 * x pfx x pfy, below 2^31 records); pinned memory from rt_host_alloc copies fastest. counts as
 * rt_render_tile. */
#define RT_SAMPLES_RGB     3
#define RT_SAMPLES_RAY_RGB 9
int rt_trace_frame_samples(rt_scene *scene, const rt_params *params, int32_t layout, float *out, size_t capacity,
                           uint64_t counts[3]);
/* Set-up without rendering: the render workspace of every pipeline a frame of params would use (tile_w x
 * tile_h tiles over the whole frame; with RT_TUNE_FRAMES_IN_FLIGHT F, all F), and with samples_layout
 * RT_SAMPLES_RGB / RT_SAMPLES_RAY_RGB the device staging of rt_trace_frame_samples. The first render of
 * such a frame then allocates nothing (a host can do this in init(), raytracing.cpp:42-73, so the first
 * 'r' press pays only the render). samples_layout 0: the workspace only. Synchronises the device's work
 * on the scene's stream. */
int rt_scene_reserve(rt_scene *scene, const rt_params *params, int32_t tile_w, int32_t tile_h, int32_t samples_layout);
/* Page-locked host memory (hipHostMalloc on the scene's device's runtime), for rt_trace_frame_samples'
 * output and other large device-to-host results. */
int  rt_host_alloc(size_t bytes, void **out);
void rt_host_free(void *ptr);
/* The whole frame, row-major (height x width x 3 bytes, the PPM's pixel order), into the DEVICE
 * buffer d_out_u8, rendered in tile_w x tile_h tiles; stream semantics as rt_render_tiles_device.
 * The single-GPU form of the shard + gather path (no un-permute needed). */
int rt_render_frame_device(rt_scene *scene, const rt_params *params, int32_t tile_w, int32_t tile_h, void *d_out_u8,
                           size_t out_capacity, void *stream, uint64_t counts[3]);
/* Several frames of one frame geometry, each its own view: params[f] (f < n_frames) may differ from
 * params[0] in their corner rays only (the trackball turned between 'r' presses, main.cpp:355-358), and
 * frame f goes row-major into the DEVICE buffer d_out_u8[f] (each out_capacity bytes). One chain launch
 * renders all of them when the frame is one batch of the four-wide tree (C4, C5, the reference's defaults): its wave tasks cycle
 * over the frames, so the frames' longest batches start side by side and the short ones of each fill
 * the slots the others' tails free, on one stream and one hardware queue (the overlap frames in flight
 * on two streams get, without depending on the runtime placing those streams on different hardware
 * queues). Otherwise the frames render one after another. Bytes equal the frames rendered one at a
 * time. counts: the sum over the frames. Stream semantics as rt_render_tiles_device. */
#define RT_MAX_FRAMES_PER_CALL 8
int rt_render_frames_device(rt_scene *scene, const rt_params *params, int32_t n_frames, int32_t tile_w, int32_t tile_h,
                            void *const *d_out_u8, size_t out_capacity, void *stream, uint64_t counts[3]);
int rt_render_tiles_device(rt_scene *scene, const rt_params *params, int32_t tile_w, int32_t tile_h,
                           int32_t frames, int32_t first, int32_t stride, void *d_out_u8, size_t out_capacity,
                           void *stream, int32_t *n_tiles_out, uint64_t counts[3]);

/* ---- multi-GPU ---------------------------------------------------------- */
/* One rank per GPU (a process or a host thread each). Rank 0 makes an id with rt_comm_unique_id
 * and the host hands its RT_COMM_ID_BYTES bytes to every rank (file, MPI, a TCP store...); every
 * rank then calls rt_comm_init (collective: it returns when all nranks have joined). RCCL
 * (librccl.so.1) is loaded on first use. */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm;
int  rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
int  rt_comm_init(int32_t device, int32_t rank, int32_t nranks, const uint8_t id[RT_COMM_ID_BYTES], rt_comm **out);
void rt_comm_destroy(rt_comm *comm);
int  rt_comm_info(const rt_comm *comm, int32_t *rank, int32_t *nranks, int32_t *device);
/* Polls the communicator (ncclCommGetAsyncError): RT_OK or RT_E_RCCL with the error's text. */
int  rt_comm_check(rt_comm *comm);
/* The 'r' loop over the communicator's GPUs. Collective: every rank calls it with the same params,
 * tiling and frame count, its scene on its own device. `frames` frames of the view are cut into
 * tile_w x tile_h tiles, ids g = f*T + t; rank r renders ids r, r+N, ... (rt_render_tiles_device),
 * ONE gather (RCCL, equal-sized shards) brings the quantised tiles to rank 0, which un-permutes them
 * on the device into d_frames_out: frames x height x width x 3 bytes, row-major, the PPM's order
 * (other ranks: d_frames_out may be NULL). Bytes equal the one-GPU render's. Asynchronous on the
 * caller's `stream` unless counts != NULL (this rank's queries per kind; then it synchronises and
 * polls the communicator). */
int rt_render_frames_sharded(rt_scene *scene, const rt_params *params, rt_comm *comm, int32_t tile_w, int32_t tile_h,
                             int32_t frames, void *d_frames_out, size_t out_capacity, void *stream, uint64_t counts[3]);
/* Pipelining of rt_render_frames_sharded (collective: every rank sets the same depth; synchronises
 * the device). depth 1 (default): render, gather and un-permute in order on the caller's stream.
 * depth 2: call i renders on the communicator's render stream i % 2 into one of two alternating
 * shard buffers and gathers + un-permutes on its exchange stream; the caller's stream waits for
 * that call's un-permute (d_frames_out is ready in stream order, as at depth 1), but the next call's
 * render does not wait for the caller's stream, so it overlaps this call's gather and un-permute,
 * and this call's render too when the scene keeps frames in flight (RT_TUNE_FRAMES_IN_FLIGHT 2).
 * The gather and un-permute still follow the caller's work queued before the call.
 * The host must then keep d_frames_out of consecutive calls distinct until its stream has passed
 * them. Calls with counts != NULL drain the pipeline and run as at depth 1. */
int rt_comm_set_pipeline(rt_comm *comm, int32_t depth);
/* The un-permute step alone: d_gathered = nranks shards of slots = ceil(frames*T / nranks) tiles
 * each (tile g in shard g % nranks, slot g / nranks; tile_w*tile_h*3 bytes per tile, row-major
 * inside the tile) -> d_frames_out as above. For hosts that gather with their own transport. */
int rt_assemble_tiles_device(int32_t device, int32_t width, int32_t height, int32_t tile_w, int32_t tile_h, int32_t frames,
                             int32_t nranks, const void *d_gathered, size_t gathered_bytes, void *d_frames_out,
                             size_t out_capacity, void *stream);

/* ---- helpers -------------------------------------------------------------------------- */
/* Corner rays of the reference's default view (camera at (0,0,4), fovy 50, near 1, far 10). */
int rt_default_corners(int32_t width, int32_t height, float corners[8][3]);
/* Image::writeImage: "P6\n%i %i\n255\n" + w*h*3 bytes. */
int rt_write_ppm(const char *path, int32_t width, int32_t height, const uint8_t *rgb_u8);
/* A host that writes result.ppm after every frame (main.cpp:405): the file opened once, sized and kept
 * mapped; rt_ppm_writer_write copies a frame's w*h*3 bytes into it with `threads` threads (1-256), slice
 * by slice, and returns when they are in the file's page-cache pages. The file then holds the bytes
 * rt_write_ppm writes. (write() of one file does not scale with threads: the kernel serialises buffered
 * writes to one inode.) */
typedef struct rt_ppm_writer rt_ppm_writer;
int rt_ppm_writer_open(const char *path, int32_t width, int32_t height, int32_t threads, rt_ppm_writer **out);
int rt_ppm_writer_write(rt_ppm_writer *w, const uint8_t *rgb_u8);
void rt_ppm_writer_close(rt_ppm_writer *w);

/* ---- acceleration ------------------------------------------------------ */
/* The reference loops over every triangle for every ray (raytracing.cpp:174-189) and leaves its
 * KD-tree commented out (:167-172). RT_ACCEL_BVH visits only triangles whose padded acceptance
 * box the ray can reach; results (index, hit point, every output byte) are identical to
 * RT_ACCEL_BRUTE_FORCE by construction. Default: RT_ACCEL_BVH. */
#define RT_ACCEL_BRUTE_FORCE 0
#define RT_ACCEL_BVH         1
int rt_scene_set_accel(rt_scene *scene, int32_t mode);
int rt_scene_get_accel(const rt_scene *scene, int32_t *mode);
/* info[0] inner nodes of the binary tree, [1] its depth, [2] always-tested (ill-conditioned)
 * triangles, [3] never-accepted (degenerate) triangles, [4] triangles in leaves, [5] nodes of the
 * four-wide tree the kernels traverse by default, [6] its depth. Builds the BVH on demand. */
#define RT_BVH_INFO_FIELDS 7
int rt_scene_bvh_info(rt_scene *scene, int32_t info[RT_BVH_INFO_FIELDS]);
/* 64-bit FNV-1a digest of the BVH arrays the device receives (both trees, leaf order, always
 * list): equal digests = identical trees (the parallel and sequential builds are compared so). */
int rt_scene_bvh_digest(rt_scene *scene, uint64_t *digest);
/* The order the builder chose, read only: leaf_tris[i] = the triangle in leaf slot i (info[4] entries),
 * always[k] = the k-th always-tested triangle (info[2] entries). The counts are written whenever the
 * pointers are valid; RT_E_ARG on a NULL pointer or a capacity below its count (nothing is copied). */
int rt_scene_bvh_order(rt_scene *scene, uint32_t *leaf_tris, int64_t leaf_capacity, int64_t *n_leaf, uint32_t *always,
                       int64_t always_capacity, int64_t *n_always);
/* Host-side structural check of the built BVH (containment, coverage, depth bound). */
int rt_scene_bvh_validate(rt_scene *scene);
/* The padded acceptance box of one triangle T = {T0, T1, T2} (9 floats), as the BVH uses it.
 * Returns 0 (box written), 1 (ill-conditioned: tested by every query) or 2 (never accepted). */
int rt_bvh_acceptance_box(const float T[9], float lo[3], float hi[3]);

/* ---- measurement ---------------------------------------------------------------------- */
/* Kernel kinds for rt_kernel_stats. */
#define RT_KERNEL_CLOSEST_HIT 0   /* closest-hit over all triangles (primary + secondary queries) */
#define RT_KERNEL_SHADOW      1   /* shadow queries (closest-hit or any-hit) */
#define RT_KERNEL_SHADE       2   /* shading / secondary-ray generation */
#define RT_KERNEL_FRAME       3   /* sample generation + fold + AA + quantise */
#define RT_KERNEL_CHAIN       4   /* closest-hit + shadows + shade of every step from chain_from on, per
                                     lane in one launch (RT_TUNE_CHAIN_FROM); tests = brute-force
                                     equivalent of all its closest-hit and shadow queries */
#define RT_KERNEL_KINDS       5
/* RT_PROFILE_TIMING: every launch of the scene is bracketed with hipEvents on its own stream and
 * the durations accumulated (one host sync per render call). RT_PROFILE_WORK additionally has the
 * BVH kernels count their work (rt_work_stats / rt_work_detail); the counting itself costs time,
 * so time and count in separate passes. */
#define RT_PROFILE_OFF    0
#define RT_PROFILE_TIMING 1
#define RT_PROFILE_WORK   2
int rt_set_profiling(rt_scene *scene, int32_t mode);
/* launches, summed milliseconds, and summed ray-triangle tests (closest-hit/shadow kinds). */
int rt_kernel_stats(rt_scene *scene, int32_t kind, uint64_t *launches, double *total_ms, double *tests);
int rt_reset_stats(rt_scene *scene);
/* Ray-triangle tests and BVH node visits executed by the BVH kernels of `kind`
 * (RT_KERNEL_CLOSEST_HIT or RT_KERNEL_SHADOW) while profiling was RT_PROFILE_WORK, since the last
 * reset (synchronises the device). */
int rt_work_stats(rt_scene *scene, int32_t kind, double *tests, double *node_visits);
/* Launch-shape tuning and the diagnostics of the tuning work (rt_scene_tune, rt_scene_trials,
 * rt_batch_durations, rt_work_detail, rt_diag_read, rt_workspace_layout) are declared in
 * raytracert_tune.h: they are not part of the drop-in contract, and no result depends on them. */

#ifdef __cplusplus
}
#endif
#endif
