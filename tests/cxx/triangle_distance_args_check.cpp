// Host check of the triangle-distance entries' argument rules (triangle_distance_args and triangle_within_args of
// raytracert_amd/csrc/query_args.h): a call in order passes, every rule broken alone gives its own message, of two
// rules adjacent in the entry's order the earlier one wins, a call that breaks them all gives the first, and
// n == 0 passes null arrays while every rule that does not depend on n still holds. Addresses are made up and
// never read. Prints "ok <rules> rules, <checks> checks" or the failed checks; run by
// tests/test_triangle_distance_capi.py, also under the host sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "query_args.h"

using namespace rt;

static int g_checks = 0, g_failed = 0;
static void expect(const char *got, const char *want, const char *entry, const char *what) {
    ++g_checks;
    if ((!got && !want) || (got && want && std::strcmp(got, want) == 0)) return;
    ++g_failed;
    std::printf("FAILED %s, %s: got \"%s\", want \"%s\"\n", entry, what, got ? got : "(null)", want ? want : "(null)");
}

struct Args {
    bool scene;
    uintptr_t tris;
    int32_t stride, n;
    uintptr_t count, rmax, self;
    uint32_t flags;
    uintptr_t hit, qpoint, point;   // (the verdict entry: hit is d_within_out)
};
static const void *ptr(uintptr_t a) { return reinterpret_cast<const void *>(a); }
static Args in_order() { return Args{true, 0x10000, RT_RAYS_PADDED, 65, 0x30000, 0x40000, 0x50000, 0, 0x60000, 0x70000, 0x80000}; }

using Break = void (*)(Args &);
struct Rule {
    const char *msg;
    std::vector<Break> breaks;   // each alone breaks this rule; the first is the one combined with other rules
    bool at_zero = true;         // still refused when n == 0
};
using Call = const char *(*)(const Args &);

static const char *distance(const Args &a) {
    return triangle_distance_args(a.scene, ptr(a.tris), a.stride, a.n, ptr(a.count), ptr(a.rmax), ptr(a.self), a.flags, ptr(a.hit),
                                  ptr(a.qpoint), ptr(a.point));
}
static const char *within(const Args &a) {
    return triangle_within_args(a.scene, ptr(a.tris), a.stride, a.n, ptr(a.count), ptr(a.rmax), ptr(a.self), a.flags, ptr(a.hit));
}

static std::vector<Rule> arrays() {
    return {{"scene is NULL", {[](Args &a) { a.scene = false; }}},
            {"n must be >= 0", {[](Args &a) { a.n = -1; }}, false},
            {"tri_stride must be 3 (packed) or 4 (padded)", {[](Args &a) { a.stride = 5; }, [](Args &a) { a.stride = 0; }, [](Args &a) { a.stride = 16; }}},
            {"triangle array is NULL", {[](Args &a) { a.tris = 0; }}, false}};
}
static const Rule kPadded{"the padded triangle array must be 16-byte aligned", {[](Args &a) { a.tris += 4; }, [](Args &a) { a.tris += 8; }}};
static const Rule kInputs{"d_count, d_rmax and d_self must be 4-byte aligned",
                          {[](Args &a) { a.count += 2; }, [](Args &a) { a.rmax += 1; }, [](Args &a) { a.self += 3; }}};
static const Rule kFlags{"flags must be 0", {[](Args &a) { a.flags = 1; }, [](Args &a) { a.flags = RT_TRI_COUNT_ALL; }, [](Args &a) { a.flags = 1u << 31; }}};

static std::vector<Rule> distance_rules() {
    std::vector<Rule> r = arrays();
    r.push_back(kPadded);
    r.push_back({"output array is NULL", {[](Args &a) { a.hit = 0; }}, false});
    r.push_back({"d_hit_out must be 16-byte aligned", {[](Args &a) { a.hit += 8; }, [](Args &a) { a.hit += 4; }}});
    r.push_back({"d_qpoint_out and d_point_out must be 4-byte aligned", {[](Args &a) { a.qpoint += 2; }, [](Args &a) { a.point += 1; }}});
    r.push_back(kInputs);
    r.push_back(kFlags);
    return r;
}
static std::vector<Rule> within_rules() {
    std::vector<Rule> r = arrays();
    r.push_back(kPadded);
    r.push_back({"output array is NULL", {[](Args &a) { a.hit = 0; }}, false});
    r.push_back(kInputs);
    r.push_back(kFlags);
    return r;
}

static int check_entry(const char *name, Call call, const std::vector<Rule> &rules, bool has_points) {
    expect(call(in_order()), nullptr, name, "a call in order");
    Args opt = in_order();                        // every optional array absent, packed and 4-byte aligned only
    opt.stride = RT_RAYS_PACKED;
    opt.tris += 4;
    opt.count = opt.rmax = opt.self = opt.qpoint = opt.point = 0;
    if (has_points) opt.hit += 16;
    else opt.hit += 1;                            // (bytes: no alignment)
    expect(call(opt), nullptr, name, "packed, optional arrays absent");
    Args mis = in_order();                        // the packed wording of the array's alignment rule
    mis.stride = RT_RAYS_PACKED;
    mis.tris += 2;
    expect(call(mis), "the triangle array must be 4-byte aligned", name, "packed array off by 2");
    for (size_t i = 0; i < rules.size(); ++i) {
        for (Break b : rules[i].breaks) {         // alone
            Args a = in_order();
            b(a);
            expect(call(a), rules[i].msg, name, rules[i].msg);
        }
        if (i + 1 < rules.size()) {               // with the next rule broken too, this one wins
            Args a = in_order();
            rules[i + 1].breaks[0](a);
            rules[i].breaks[0](a);                // (last: where both change one address, this rule's value stands)
            expect(call(a), rules[i].msg, name, "before the next rule");
        }
        Args z = in_order();                      // n == 0
        z.n = 0;
        z.tris = z.hit = 0;
        rules[i].breaks[0](z);
        if (std::strcmp(rules[i].msg, "n must be >= 0") != 0) expect(call(z), rules[i].at_zero ? rules[i].msg : nullptr, name, "n == 0");
    }
    Args all = in_order();                        // everything broken: the first rule
    for (size_t i = rules.size(); i-- > 0;) rules[i].breaks[0](all);
    expect(call(all), rules[0].msg, name, "every rule broken");
    Args zero = in_order();
    zero.n = 0;
    zero.tris = zero.hit = zero.qpoint = zero.point = zero.count = zero.rmax = zero.self = 0;
    expect(call(zero), nullptr, name, "n == 0 with null arrays");
    return static_cast<int>(rules.size());
}

int main() {
    int rules = check_entry("rt_triangle_distance_device", distance, distance_rules(), true);
    rules += check_entry("rt_triangle_within_device", within, within_rules(), false);
    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    std::printf("ok %d rules, %d checks\n", rules, g_checks);
    return 0;
}
