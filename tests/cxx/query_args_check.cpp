// Host check of the device-resident query entries' argument rules (raytracert_amd/csrc/query_args.h): per
// entry a call in order passes, every rule broken alone gives its own message, of two rules adjacent in the
// entry's order the earlier one wins, a call that breaks them all gives the first, and n == 0 passes null
// arrays while every rule that does not depend on n still holds. The messages and their order are written
// out here as rt_capi.cpp had them inline before the header existed. Addresses are made up and never read.
// Prints "ok <rules> rules, <checks> checks" or the failed checks; run by tests/test_query_args.py, also
// under the host sanitizers.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "query_args.h"

using namespace rt;

static int g_checks = 0, g_failed = 0;
static const char *g_entry = "";
static void expect(const char *got, const char *want, const char *what, const char *rule) {
    ++g_checks;
    const bool same = (!got && !want) || (got && want && std::strcmp(got, want) == 0);
    if (same) return;
    ++g_failed;
    std::printf("FAILED %s, %s [%s]: got \"%s\", want \"%s\"\n", g_entry, what, rule ? rule : "-", got ? got : "(null)", want ? want : "(null)");
}

// Every entry's arguments: two input arrays, d_count, two more per-query inputs (tmin or rmax or after; tmax or
// self), three outputs. An entry reads the ones it has.
struct Args {
    bool scene;
    uintptr_t in0, in1;
    int32_t stride, n;
    uintptr_t count, aux0, aux1;
    uint32_t flags;
    int32_t k, axis;
    uintptr_t out0, out1, out2;
};
static const void *ptr(uintptr_t a) { return reinterpret_cast<const void *>(a); }
static Args in_order() {   // padded arrays, every pointer 16-byte aligned
    return Args{true, 0x10000, 0x20000, RT_RAYS_PADDED, 65, 0x30000, 0x40000, 0x50000, 0, 4, RT_AXIS_POS_Z, 0x60000, 0x70000, 0x80000};
}

using Break = void (*)(Args &);
enum Field { kNone, kIn0, kIn1, kCount, kAux0, kAux1, kOut0, kOut1, kOut2 };
struct Rule {
    const char *msg;
    std::vector<Break> breaks;   // each alone breaks this rule; the first is the one combined with other rules
    Field field = kNone;         // what the first one changes: two rules on one field cannot both be broken
    bool at_zero = true;         // still refused when n == 0
    const char *packed_msg = nullptr;   // the alignment rule's wording at stride 3 ...
    Break packed_break = nullptr;       // ... and what breaks it there
};
struct Entry {
    const char *name;
    const char *(*call)(const Args &);
    std::vector<Rule> rules;     // in the entry's order
};

// ---- the rules, in the words of the C ABI ----
static Rule no_scene() { return {"scene is NULL", {[](Args &a) { a.scene = false; }}}; }
static Rule negative_n() { return {"n must be >= 0", {[](Args &a) { a.n = -1; }}, kNone, false}; }
static Rule bad_stride(const char *msg) { return {msg, {[](Args &a) { a.stride = 5; }, [](Args &a) { a.stride = 0; }, [](Args &a) { a.stride = 16; }}}; }
static const Break kMisIn0 = [](Args &a) { a.in0 += 4; };
static const Break kMisIn1 = [](Args &a) { a.in1 += 4; };
static const Break kPackedMisIn0 = [](Args &a) { a.stride = RT_RAYS_PACKED; a.in0 += 2; };
static const Break kPackedMisIn1 = [](Args &a) { a.stride = RT_RAYS_PACKED; a.in1 += 2; };
static std::vector<Rule> two_arrays(const char *stride, const char *null, const char *padded, const char *packed) {
    return {no_scene(), negative_n(), bad_stride(stride),
            {null, {[](Args &a) { a.in0 = 0; }, [](Args &a) { a.in1 = 0; }}, kIn0, false},
            {padded, {kMisIn1, kMisIn0}, kIn1, true, packed, kPackedMisIn1}};
}
static std::vector<Rule> one_array(const char *stride, const char *null, const char *padded, const char *packed) {
    return {no_scene(), negative_n(), bad_stride(stride),
            {null, {[](Args &a) { a.in0 = 0; }}, kIn0, false},
            {padded, {kMisIn0}, kIn0, true, packed, kPackedMisIn0}};
}
static std::vector<Rule> rays() {
    return two_arrays("ray_stride must be 3 (packed) or 4 (padded)", "ray array is NULL", "padded ray arrays must be 16-byte aligned",
                      "ray arrays must be 4-byte aligned");
}
static std::vector<Rule> points() {
    return one_array("point_stride must be 3 (packed) or 4 (padded)", "point array is NULL", "padded point arrays must be 16-byte aligned",
                     "point arrays must be 4-byte aligned");
}
static std::vector<Rule> boxes() {
    return two_arrays("box_stride must be 3 (packed) or 4 (padded)", "box array is NULL", "padded box arrays must be 16-byte aligned",
                      "box arrays must be 4-byte aligned");
}
static std::vector<Rule> tris() {
    return one_array("tri_stride must be 3 (packed) or 4 (padded)", "triangle array is NULL", "the padded triangle array must be 16-byte aligned",
                     "the triangle array must be 4-byte aligned");
}

static const Break kMisCount = [](Args &a) { a.count += 2; };
static const Break kMisAux0 = [](Args &a) { a.aux0 += 2; };
static const Break kMisAux1 = [](Args &a) { a.aux1 += 2; };
static const Break kMisOut0 = [](Args &a) { a.out0 += 2; };
static const Break kMisOut1 = [](Args &a) { a.out1 += 2; };
static const Break kMisOut2 = [](Args &a) { a.out2 += 2; };
static Rule null_out0() { return {"output array is NULL", {[](Args &a) { a.out0 = 0; }}, kOut0, false}; }
static Rule record_aligned(const char *msg) {   // 16-byte records: 4- and 8-byte aligned addresses are refused too
    return {msg, {[](Args &a) { a.out0 += 4; }, [](Args &a) { a.out0 += 8; }, kMisOut0}, kOut0};
}
static Rule bad_k() { return {"k must be in [1, RT_MULTI_HIT_MAX]", {[](Args &a) { a.k = 0; }, [](Args &a) { a.k = RT_MULTI_HIT_MAX + 1; }, [](Args &a) { a.k = -1; }}}; }
static Rule list_too_long() {
    return {"n * k exceeds INT32_MAX (split the batch)", {[](Args &a) { a.n = INT32_MAX / RT_MULTI_HIT_MAX + 1; a.k = RT_MULTI_HIT_MAX; }}, kNone, false};
}
static Rule flags_zero() { return {"flags must be 0", {[](Args &a) { a.flags |= 1u; }, [](Args &a) { a.flags |= 1u << 31; }}}; }
static Rule bad_axis() { return {"axis must be RT_AXIS_POS_X .. RT_AXIS_NEG_Z", {[](Args &a) { a.axis = -1; }, [](Args &a) { a.axis = 6; }}}; }
static void append(std::vector<Rule> &to, std::vector<Rule> more) { to.insert(to.end(), more.begin(), more.end()); }
// check_range_args; unused: a range flag that the entry at hand does not take
static std::vector<Rule> range_rules(Break unused) {
    return {{"d_count, d_tmin and d_tmax must be 4-byte aligned", {kMisCount, kMisAux0, kMisAux1}, kCount},
            {"unknown flag bits", {[](Args &a) { a.flags |= 1u << 20; }, [](Args &a) { a.flags |= RT_NEAR_COUNT_ALL; }}},
            {"a flag this entry does not use", {unused}}};
}
// check_point_args after the point array's rules
static std::vector<Rule> closest_point_rules() {
    return {null_out0(), record_aligned("d_hit_out must be 16-byte aligned"), {"d_point_out must be 4-byte aligned", {kMisOut1}, kOut1},
            {"d_count and d_rmax must be 4-byte aligned", {kMisCount, kMisAux0}, kCount}, flags_zero()};
}
// the list entries' flag rules: any flag but the entry's own (other: one such bit), then that flag without its array
static Rule only_flag(Break other) { return {"unknown flag, or one this entry does not use", {other, [](Args &a) { a.flags |= 1u << 20; }}}; }
static Rule needs_counts(const char *msg, Break set) { return {msg, {set}, kOut1}; }

static std::vector<Entry> entries() {
    std::vector<Entry> e;
    {
        Entry x{"rt_intersect_mesh_device", [](const Args &a) {
                    return intersect_mesh_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), ptr(a.out0), ptr(a.out1));
                }, rays()};
        append(x.rules, {{"output array is NULL", {[](Args &a) { a.out0 = 0; }, [](Args &a) { a.out1 = 0; }}, kOut0, false},
                         {"d_count and the output arrays must be 4-byte aligned", {kMisCount, kMisOut0, kMisOut1}, kCount}});
        e.push_back(x);
    }
    {
        Entry x{"rt_occluded_device", [](const Args &a) {
                    return occluded_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), ptr(a.out0));
                }, rays()};
        append(x.rules, {null_out0(), {"d_count must be 4-byte aligned", {kMisCount}, kCount}});
        e.push_back(x);
    }
    {
        Entry x{"rt_closest_hit_range_device", [](const Args &a) {
                    return closest_hit_range_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), ptr(a.aux0), ptr(a.aux1), a.flags,
                                                  ptr(a.out0), ptr(a.out1));
                }, rays()};
        append(x.rules, {null_out0(), record_aligned("d_hit_out must be 16-byte aligned"), {"d_point_out must be 4-byte aligned", {kMisOut1}, kOut1}});
        append(x.rules, range_rules([](Args &a) { a.flags |= RT_OCCLUDE_ANY_OPAQUE; }));
        x.rules.back().breaks.push_back([](Args &a) { a.flags |= RT_MULTI_COUNT_ALL; });
        e.push_back(x);
    }
    {
        Entry x{"rt_occluded_range_device", [](const Args &a) {
                    return occluded_range_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), ptr(a.aux0), ptr(a.aux1), a.flags,
                                               ptr(a.out0));
                }, rays()};
        append(x.rules, {null_out0()});
        append(x.rules, range_rules([](Args &a) { a.flags |= RT_MULTI_COUNT_ALL; }));
        e.push_back(x);
    }
    {
        Entry x{"rt_multi_hit_range_device", [](const Args &a) {
                    return multi_hit_range_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), ptr(a.aux0), ptr(a.aux1), a.flags, a.k,
                                                ptr(a.out0), ptr(a.out1));
                }, rays()};
        append(x.rules, {bad_k(), null_out0(), record_aligned("d_hits_out must be 16-byte aligned"),
                         {"d_nhits_out must be 4-byte aligned", {kMisOut1}, kOut1}});
        append(x.rules, range_rules([](Args &a) { a.flags |= RT_OCCLUDE_ANY_OPAQUE; }));
        append(x.rules, {needs_counts("RT_MULTI_COUNT_ALL needs d_nhits_out", [](Args &a) { a.flags |= RT_MULTI_COUNT_ALL; a.out1 = 0; }), list_too_long()});
        e.push_back(x);
    }
    {
        Entry x{"rt_closest_point_device", [](const Args &a) {
                    return check_point_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), ptr(a.aux0), a.flags, ptr(a.out0), ptr(a.out1));
                }, points()};
        append(x.rules, closest_point_rules());
        e.push_back(x);
    }
    {
        Entry x{"rt_nearest_triangles_device", [](const Args &a) {
                    return nearest_triangles_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), ptr(a.aux0), a.flags, a.k, ptr(a.out0), ptr(a.out1),
                                                  ptr(a.out2));
                }, points()};
        append(x.rules, {bad_k(), null_out0(), record_aligned("d_hits_out must be 16-byte aligned"),
                         {"d_nfound_out must be 4-byte aligned", {kMisOut1}, kOut1}, {"d_points_out must be 4-byte aligned", {kMisOut2}, kOut2},
                         {"d_count and d_rmax must be 4-byte aligned", {kMisCount, kMisAux0}, kCount},
                         only_flag([](Args &a) { a.flags |= RT_RANGE_TO_DEST; }),
                         needs_counts("RT_NEAR_COUNT_ALL needs d_nfound_out", [](Args &a) { a.flags |= RT_NEAR_COUNT_ALL; a.out1 = 0; }), list_too_long()});
        e.push_back(x);
    }
    {
        Entry x{"rt_within_radius_device", [](const Args &a) {
                    return within_radius_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), ptr(a.aux0), a.flags, ptr(a.out0));
                }, points()};
        append(x.rules, {null_out0(), {"d_count and d_rmax must be 4-byte aligned", {kMisCount, kMisAux0}, kCount}, flags_zero()});
        e.push_back(x);
    }
    {
        Entry x{"rt_point_inside_device", [](const Args &a) {
                    return point_inside_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), a.axis, a.flags, ptr(a.out0), ptr(a.out1));
                }, points()};
        append(x.rules, {null_out0(), {"d_crossings_out must be 4-byte aligned", {kMisOut1}, kOut1}, {"d_count must be 4-byte aligned", {kMisCount}, kCount},
                         flags_zero(), bad_axis()});
        e.push_back(x);
    }
    {
        Entry x{"rt_signed_distance_device", [](const Args &a) {
                    return signed_distance_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), ptr(a.aux0), a.axis, a.flags, ptr(a.out0), ptr(a.out1));
                }, points()};
        append(x.rules, closest_point_rules());
        append(x.rules, {bad_axis()});
        e.push_back(x);
    }
    {
        Entry x{"rt_box_overlap_device", [](const Args &a) {
                    return box_overlap_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), ptr(a.aux0), a.flags, a.k, ptr(a.out0), ptr(a.out1));
                }, boxes()};
        append(x.rules, {bad_k(), null_out0(), {"d_tris_out must be 4-byte aligned", {kMisOut0}, kOut0}, {"d_nfound_out must be 4-byte aligned", {kMisOut1}, kOut1},
                         {"d_count and d_after must be 4-byte aligned", {kMisCount, kMisAux0}, kCount}, only_flag([](Args &a) { a.flags |= RT_NEAR_COUNT_ALL; }),
                         needs_counts("RT_BOX_COUNT_ALL needs d_nfound_out", [](Args &a) { a.flags |= RT_BOX_COUNT_ALL; a.out1 = 0; }), list_too_long()});
        e.push_back(x);
    }
    {
        Entry x{"rt_box_occupied_device", [](const Args &a) {
                    return box_occupied_args(a.scene, ptr(a.in0), ptr(a.in1), a.stride, a.n, ptr(a.count), a.flags, ptr(a.out0));
                }, boxes()};
        append(x.rules, {null_out0(), {"d_count must be 4-byte aligned", {kMisCount}, kCount}, flags_zero()});
        e.push_back(x);
    }
    {
        Entry x{"rt_triangle_overlap_device", [](const Args &a) {
                    return triangle_overlap_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), ptr(a.aux0), ptr(a.aux1), a.flags, a.k, ptr(a.out0),
                                                 ptr(a.out1));
                }, tris()};
        append(x.rules, {bad_k(), null_out0(), {"d_tris_out must be 4-byte aligned", {kMisOut0}, kOut0}, {"d_nfound_out must be 4-byte aligned", {kMisOut1}, kOut1},
                         {"d_count, d_after and d_self must be 4-byte aligned", {kMisCount, kMisAux0, kMisAux1}, kCount},
                         only_flag([](Args &a) { a.flags |= RT_NEAR_COUNT_ALL; }),
                         needs_counts("RT_TRI_COUNT_ALL needs d_nfound_out", [](Args &a) { a.flags |= RT_TRI_COUNT_ALL; a.out1 = 0; }), list_too_long()});
        e.push_back(x);
    }
    {
        Entry x{"rt_triangle_collides_device", [](const Args &a) {
                    return triangle_collides_args(a.scene, ptr(a.in0), a.stride, a.n, ptr(a.count), ptr(a.aux1), a.flags, ptr(a.out0));
                }, tris()};
        append(x.rules, {null_out0(), {"d_count and d_self must be 4-byte aligned", {kMisCount, kMisAux1}, kCount}, flags_zero()});
        e.push_back(x);
    }
    return e;
}

static int check_entry(const Entry &e) {
    g_entry = e.name;
    const std::vector<Rule> &r = e.rules;
    // (1) in order: padded and packed, with and without the optional arrays
    expect(e.call(in_order()), nullptr, "a call in order", nullptr);
    Args a = in_order();
    a.stride = RT_RAYS_PACKED;
    a.in0 += 4; a.in1 += 4;           // packed arrays need 4-byte alignment only
    a.count = a.aux0 = a.aux1 = 0;    // (optional in every entry)
    expect(e.call(a), nullptr, "a packed call without the optional arrays", nullptr);
    // (2) each rule alone, by each of its breaks
    for (const Rule &x : r) {
        for (Break b : x.breaks) {
            a = in_order();
            b(a);
            expect(e.call(a), x.msg, "broken alone", x.msg);
        }
        if (x.packed_break) {
            a = in_order();
            x.packed_break(a);
            expect(e.call(a), x.packed_msg, "broken alone, packed", x.packed_msg);
        }
    }
    // (3) precedence: of two adjacent rules the earlier wins; with all broken, the first
    for (size_t i = 0; i + 1 < r.size(); ++i) {
        if (r[i].field != kNone && r[i].field == r[i + 1].field) continue;   // (one pointer cannot be both null and misaligned)
        a = in_order();
        r[i + 1].breaks[0](a);
        r[i].breaks[0](a);
        expect(e.call(a), r[i].msg, "broken with the rule after it", r[i].msg);
    }
    a = in_order();
    for (size_t i = r.size(); i-- > 0;) r[i].breaks[0](a);
    expect(e.call(a), r[0].msg, "all rules broken", r[0].msg);
    // the list's size at the limit: the largest n for k = RT_MULTI_HIT_MAX and n * k == INT32_MAX (a prime: k = 1) pass
    if (std::strcmp(r.back().msg, "n * k exceeds INT32_MAX (split the batch)") == 0) {
        a = in_order();
        a.k = RT_MULTI_HIT_MAX;
        a.n = INT32_MAX / RT_MULTI_HIT_MAX;
        expect(e.call(a), nullptr, "the largest n for the largest k", nullptr);
        a.n += 1;
        expect(e.call(a), r.back().msg, "one more than the largest n for the largest k", r.back().msg);
        a.k = 1;
        a.n = INT32_MAX;
        expect(e.call(a), nullptr, "n * k == INT32_MAX", nullptr);
        a.k = 2;
        a.n = INT32_MAX / 2 + 1;
        expect(e.call(a), r.back().msg, "n * k == INT32_MAX + 1", r.back().msg);
    }
    // (4) n == 0: null arrays pass; a rule that does not depend on n is still applied
    Args zero = in_order();
    zero.n = 0;
    zero.in0 = zero.in1 = zero.count = zero.aux0 = zero.aux1 = zero.out0 = zero.out1 = zero.out2 = 0;
    expect(e.call(zero), nullptr, "n == 0 with null arrays", nullptr);
    for (const Rule &x : r) {
        for (Break b : x.breaks) {
            a = zero;
            b(a);
            a.n = 0;
            if (x.at_zero) expect(e.call(a), x.msg, "n == 0, broken", x.msg);
        }
    }
    return static_cast<int>(r.size());
}

int main() {
    int rules = 0;
    for (const Entry &e : entries()) rules += check_entry(e);
    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    std::printf("ok %d rules, %d checks\n", rules, g_checks);
    return 0;
}
