// query_args.h — what the device-resident query entries of rt_capi.cpp refuse, and in which order (the first
// rule a call breaks is the error its caller sees). Each entry has one function here that applies its rules
// to the entry's own arguments and returns the message of the first one broken, or null; rt_capi.cpp turns a
// message into RT_E_ARG. Addresses are compared, never read, and nothing here touches HIP or the scene (it
// is "is there one"), so tests/cxx/query_args_check.cpp drives every rule on the host. The host-only refusal
// (RT_E_NODEV) comes before all of these, in rt_capi.cpp. n == 0 passes null arrays and skips no other rule.
#pragma once

#include <cstddef>
#include <cstdint>

#include "raytracert.h"

namespace rt {

inline bool misaligned(const void *p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

// The scene and the input arrays of one family (rays, points, boxes, query triangles), in the family's words.
// b: the family's second array, or a again.
struct ArrayWords { const char *stride, *null, *padded, *packed; };
constexpr ArrayWords kRayWords{"ray_stride must be 3 (packed) or 4 (padded)", "ray array is NULL",
                               "padded ray arrays must be 16-byte aligned", "ray arrays must be 4-byte aligned"};
constexpr ArrayWords kPointWords{"point_stride must be 3 (packed) or 4 (padded)", "point array is NULL",
                                 "padded point arrays must be 16-byte aligned", "point arrays must be 4-byte aligned"};
constexpr ArrayWords kBoxWords{"box_stride must be 3 (packed) or 4 (padded)", "box array is NULL",
                               "padded box arrays must be 16-byte aligned", "box arrays must be 4-byte aligned"};
constexpr ArrayWords kTriWords{"tri_stride must be 3 (packed) or 4 (padded)", "triangle array is NULL",
                               "the padded triangle array must be 16-byte aligned", "the triangle array must be 4-byte aligned"};
inline const char *check_arrays(const ArrayWords &w, bool scene, const void *a, const void *b, int32_t stride, int32_t n) {
    if (!scene) return "scene is NULL";
    if (n < 0) return "n must be >= 0";
    if (stride != RT_RAYS_PACKED && stride != RT_RAYS_PADDED) return w.stride;
    if (n && (!a || !b)) return w.null;
    const size_t align = stride == RT_RAYS_PADDED ? 16 : 4;
    if (misaligned(a, align) || misaligned(b, align)) return stride == RT_RAYS_PADDED ? w.padded : w.packed;
    return nullptr;
}

// The list entries' rules (after their arrays'): k, the list and its count array, then `own` (the message of
// the entry's own rules that sit between, or null), the flags, the count flag's array and the list's size.
// `own` is evaluated by the caller, before the call: the rules are pure, so only the order of the returns below
// decides which message wins. Where `own` already holds a flag rule (the multi-hit entry: check_range_args has
// refused every flag outside `known` with its own two messages), the flag rule here cannot fire for that entry.
struct ListWords { size_t out_align; const char *out_aligned, *cnt_aligned, *flag_needs_cnt; };
inline const char *check_list(const ListWords &w, int32_t n, int32_t k, const void *out, const void *cnt, const char *own,
                              uint32_t flags, uint32_t known, uint32_t count_flag) {
    if (k < 1 || k > RT_MULTI_HIT_MAX) return "k must be in [1, RT_MULTI_HIT_MAX]";
    if (n && !out) return "output array is NULL";
    if (misaligned(out, w.out_align)) return w.out_aligned;
    if (misaligned(cnt, 4)) return w.cnt_aligned;
    if (own) return own;
    if (flags & ~known) return "unknown flag, or one this entry does not use";
    if ((flags & count_flag) && !cnt) return w.flag_needs_cnt;
    if (static_cast<int64_t>(n) * k > INT32_MAX) return "n * k exceeds INT32_MAX (split the batch)";
    return nullptr;
}

// The ranged entries' own rules: the bounds' alignment and the flags.
inline const char *check_range_args(const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags, uint32_t known) {
    if (misaligned(d_count, 4) || misaligned(d_tmin, 4) || misaligned(d_tmax, 4)) return "d_count, d_tmin and d_tmax must be 4-byte aligned";
    if (flags & ~(RT_RANGE_TO_DEST | RT_OCCLUDE_ANY_OPAQUE | RT_MULTI_COUNT_ALL)) return "unknown flag bits";
    if (flags & ~known) return "a flag this entry does not use";
    return nullptr;
}

// rt_closest_point_device's rules, in the ranged entries' order; the signed-distance entry's begin with them.
inline const char *check_point_args(bool scene, const void *d_points, int32_t point_stride, int32_t n, const void *d_count,
                                    const void *d_rmax, uint32_t flags, const void *d_hit_out, const void *d_point_out) {
    if (const char *m = check_arrays(kPointWords, scene, d_points, d_points, point_stride, n)) return m;
    if (n && !d_hit_out) return "output array is NULL";
    if (misaligned(d_hit_out, sizeof(rt_hit))) return "d_hit_out must be 16-byte aligned";
    if (misaligned(d_point_out, 4)) return "d_point_out must be 4-byte aligned";
    if (misaligned(d_count, 4) || misaligned(d_rmax, 4)) return "d_count and d_rmax must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return nullptr;
}

inline const char *check_axis(int32_t axis) {
    return axis < RT_AXIS_POS_X || axis > RT_AXIS_NEG_Z ? "axis must be RT_AXIS_POS_X .. RT_AXIS_NEG_Z" : nullptr;
}

// ---- the other entries: rt_<name>_device's rules are <name>_args ----
inline const char *intersect_mesh_args(bool scene, const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n,
                                       const void *d_count, const void *d_index_out, const void *d_point_out) {
    if (const char *m = check_arrays(kRayWords, scene, d_origins, d_dests, ray_stride, n)) return m;
    if (n && (!d_index_out || !d_point_out)) return "output array is NULL";
    if (misaligned(d_count, 4) || misaligned(d_index_out, 4) || misaligned(d_point_out, 4))
        return "d_count and the output arrays must be 4-byte aligned";
    return nullptr;
}

inline const char *occluded_args(bool scene, const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n,
                                 const void *d_count, const void *d_blocked_out) {
    if (const char *m = check_arrays(kRayWords, scene, d_origins, d_dests, ray_stride, n)) return m;
    if (n && !d_blocked_out) return "output array is NULL";
    if (misaligned(d_count, 4)) return "d_count must be 4-byte aligned";
    return nullptr;
}

inline const char *closest_hit_range_args(bool scene, const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n,
                                          const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags,
                                          const void *d_hit_out, const void *d_point_out) {
    if (const char *m = check_arrays(kRayWords, scene, d_origins, d_dests, ray_stride, n)) return m;
    if (n && !d_hit_out) return "output array is NULL";
    if (misaligned(d_hit_out, sizeof(rt_hit))) return "d_hit_out must be 16-byte aligned";
    if (misaligned(d_point_out, 4)) return "d_point_out must be 4-byte aligned";
    return check_range_args(d_count, d_tmin, d_tmax, flags, RT_RANGE_TO_DEST);
}

inline const char *occluded_range_args(bool scene, const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n,
                                       const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags,
                                       const void *d_blocked_out) {
    if (const char *m = check_arrays(kRayWords, scene, d_origins, d_dests, ray_stride, n)) return m;
    if (n && !d_blocked_out) return "output array is NULL";
    return check_range_args(d_count, d_tmin, d_tmax, flags, RT_RANGE_TO_DEST | RT_OCCLUDE_ANY_OPAQUE);
}

inline const char *multi_hit_range_args(bool scene, const void *d_origins, const void *d_dests, int32_t ray_stride, int32_t n,
                                        const void *d_count, const void *d_tmin, const void *d_tmax, uint32_t flags, int32_t k,
                                        const void *d_hits_out, const void *d_nhits_out) {
    if (const char *m = check_arrays(kRayWords, scene, d_origins, d_dests, ray_stride, n)) return m;
    const uint32_t known = RT_RANGE_TO_DEST | RT_MULTI_COUNT_ALL;   // (check_range_args has refused the rest before check_list looks)
    return check_list({sizeof(rt_hit), "d_hits_out must be 16-byte aligned", "d_nhits_out must be 4-byte aligned",
                       "RT_MULTI_COUNT_ALL needs d_nhits_out"},
                      n, k, d_hits_out, d_nhits_out, check_range_args(d_count, d_tmin, d_tmax, flags, known), flags, known,
                      RT_MULTI_COUNT_ALL);
}

inline const char *nearest_triangles_args(bool scene, const void *d_points, int32_t point_stride, int32_t n, const void *d_count,
                                          const void *d_rmax, uint32_t flags, int32_t k, const void *d_hits_out,
                                          const void *d_nfound_out, const void *d_points_out) {
    if (const char *m = check_arrays(kPointWords, scene, d_points, d_points, point_stride, n)) return m;
    const char *own = misaligned(d_points_out, 4)                          ? "d_points_out must be 4-byte aligned"
                      : misaligned(d_count, 4) || misaligned(d_rmax, 4)    ? "d_count and d_rmax must be 4-byte aligned"
                                                                           : nullptr;
    return check_list({sizeof(rt_hit), "d_hits_out must be 16-byte aligned", "d_nfound_out must be 4-byte aligned",
                       "RT_NEAR_COUNT_ALL needs d_nfound_out"},
                      n, k, d_hits_out, d_nfound_out, own, flags, RT_NEAR_COUNT_ALL, RT_NEAR_COUNT_ALL);
}

inline const char *within_radius_args(bool scene, const void *d_points, int32_t point_stride, int32_t n, const void *d_count,
                                      const void *d_rmax, uint32_t flags, const void *d_within_out) {
    if (const char *m = check_arrays(kPointWords, scene, d_points, d_points, point_stride, n)) return m;
    if (n && !d_within_out) return "output array is NULL";
    if (misaligned(d_count, 4) || misaligned(d_rmax, 4)) return "d_count and d_rmax must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return nullptr;
}

inline const char *point_inside_args(bool scene, const void *d_points, int32_t point_stride, int32_t n, const void *d_count,
                                     int32_t axis, uint32_t flags, const void *d_inside_out, const void *d_crossings_out) {
    if (const char *m = check_arrays(kPointWords, scene, d_points, d_points, point_stride, n)) return m;
    if (n && !d_inside_out) return "output array is NULL";
    if (misaligned(d_crossings_out, 4)) return "d_crossings_out must be 4-byte aligned";
    if (misaligned(d_count, 4)) return "d_count must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return check_axis(axis);
}

inline const char *signed_distance_args(bool scene, const void *d_points, int32_t point_stride, int32_t n, const void *d_count,
                                        const void *d_rmax, int32_t axis, uint32_t flags, const void *d_hit_out,
                                        const void *d_point_out) {
    if (const char *m = check_point_args(scene, d_points, point_stride, n, d_count, d_rmax, flags, d_hit_out, d_point_out)) return m;
    return check_axis(axis);
}

inline const char *box_overlap_args(bool scene, const void *d_lo, const void *d_hi, int32_t box_stride, int32_t n, const void *d_count,
                                    const void *d_after, uint32_t flags, int32_t k, const void *d_tris_out, const void *d_nfound_out) {
    if (const char *m = check_arrays(kBoxWords, scene, d_lo, d_hi, box_stride, n)) return m;
    const char *own = misaligned(d_count, 4) || misaligned(d_after, 4) ? "d_count and d_after must be 4-byte aligned" : nullptr;
    return check_list({4, "d_tris_out must be 4-byte aligned", "d_nfound_out must be 4-byte aligned", "RT_BOX_COUNT_ALL needs d_nfound_out"},
                      n, k, d_tris_out, d_nfound_out, own, flags, RT_BOX_COUNT_ALL, RT_BOX_COUNT_ALL);
}

inline const char *box_occupied_args(bool scene, const void *d_lo, const void *d_hi, int32_t box_stride, int32_t n, const void *d_count,
                                     uint32_t flags, const void *d_occupied_out) {
    if (const char *m = check_arrays(kBoxWords, scene, d_lo, d_hi, box_stride, n)) return m;
    if (n && !d_occupied_out) return "output array is NULL";
    if (misaligned(d_count, 4)) return "d_count must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return nullptr;
}

inline const char *triangle_overlap_args(bool scene, const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count,
                                         const void *d_after, const void *d_self, uint32_t flags, int32_t k, const void *d_tris_out,
                                         const void *d_nfound_out) {
    if (const char *m = check_arrays(kTriWords, scene, d_qtris, d_qtris, tri_stride, n)) return m;
    const char *own = misaligned(d_count, 4) || misaligned(d_after, 4) || misaligned(d_self, 4)
                          ? "d_count, d_after and d_self must be 4-byte aligned" : nullptr;
    return check_list({4, "d_tris_out must be 4-byte aligned", "d_nfound_out must be 4-byte aligned", "RT_TRI_COUNT_ALL needs d_nfound_out"},
                      n, k, d_tris_out, d_nfound_out, own, flags, RT_TRI_COUNT_ALL, RT_TRI_COUNT_ALL);
}

inline const char *triangle_collides_args(bool scene, const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count,
                                          const void *d_self, uint32_t flags, const void *d_collides_out) {
    if (const char *m = check_arrays(kTriWords, scene, d_qtris, d_qtris, tri_stride, n)) return m;
    if (n && !d_collides_out) return "output array is NULL";
    if (misaligned(d_count, 4) || misaligned(d_self, 4)) return "d_count and d_self must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return nullptr;
}

// The triangle entries' arrays, then the closest-point entry's rules for the record and the points.
inline const char *triangle_distance_args(bool scene, const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count,
                                          const void *d_rmax, const void *d_self, uint32_t flags, const void *d_hit_out,
                                          const void *d_qpoint_out, const void *d_point_out) {
    if (const char *m = check_arrays(kTriWords, scene, d_qtris, d_qtris, tri_stride, n)) return m;
    if (n && !d_hit_out) return "output array is NULL";
    if (misaligned(d_hit_out, sizeof(rt_hit))) return "d_hit_out must be 16-byte aligned";
    if (misaligned(d_qpoint_out, 4) || misaligned(d_point_out, 4)) return "d_qpoint_out and d_point_out must be 4-byte aligned";
    if (misaligned(d_count, 4) || misaligned(d_rmax, 4) || misaligned(d_self, 4)) return "d_count, d_rmax and d_self must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return nullptr;
}

inline const char *triangle_within_args(bool scene, const void *d_qtris, int32_t tri_stride, int32_t n, const void *d_count,
                                        const void *d_rmax, const void *d_self, uint32_t flags, const void *d_within_out) {
    if (const char *m = check_arrays(kTriWords, scene, d_qtris, d_qtris, tri_stride, n)) return m;
    if (n && !d_within_out) return "output array is NULL";
    if (misaligned(d_count, 4) || misaligned(d_rmax, 4) || misaligned(d_self, 4)) return "d_count, d_rmax and d_self must be 4-byte aligned";
    if (flags) return "flags must be 0";
    return nullptr;
}

}  // namespace rt
