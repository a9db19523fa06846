// lbvh_shared.h — the integer and binary64 definitions of the Morton-order radix tree (LBVH, Karras
// 2012) that the host statement (bvh.cpp build_lbvh) and the kernels (rt_kernels.hip k_lbvh_*) must
// perform identically: both include this text, so the two builders cannot drift apart. Only IEEE
// binary64 + - * / and integer operations are used (both sides are compiled without contraction).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RT_LBVH_HD __host__ __device__ inline
#else
#define RT_LBVH_HD inline
#endif

namespace rt {

// Float bit patterns mapped so that unsigned integer order is the floats' order (-0 below +0): an
// integer min / max over these is an exact, order-independent float min / max.
RT_LBVH_HD uint32_t lbvh_ordered(uint32_t float_bits) { return (float_bits & 0x80000000u) ? ~float_bits : (float_bits | 0x80000000u); }
RT_LBVH_HD uint32_t lbvh_unordered(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// Cell of centroid coordinate c on an axis whose centroids span [cmin, cmax]: 10 bits over the axis'
// own extent; a zero (or non-finite) extent maps to cell 0.
RT_LBVH_HD uint32_t lbvh_cell(float c, float cmin, float cmax) {
    const double e = double(cmax) - double(cmin);
    if (!(e > 0)) return 0;
    const double f = (double(c) - double(cmin)) / e * 1024.0;
    return f >= 1023.0 ? 1023u : (f > 0 ? static_cast<uint32_t>(static_cast<int32_t>(f)) : 0u);
}

RT_LBVH_HD uint32_t lbvh_spread(uint32_t v) {   // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
RT_LBVH_HD uint32_t lbvh_code(uint32_t qx, uint32_t qy, uint32_t qz) { return (lbvh_spread(qx) << 2) | (lbvh_spread(qy) << 1) | lbvh_spread(qz); }

// Karras' delta over the sorted codes: common prefix length, ties broken by position (equal codes:
// 32 + clz(i ^ j)); -1 outside [0, n).
RT_LBVH_HD int lbvh_delta(const uint32_t *codes, int32_t n, int32_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t a = codes[i], b = codes[j];
    if (a != b) return __builtin_clz(a ^ b);
    return 32 + __builtin_clz(static_cast<uint32_t>(i) ^ static_cast<uint32_t>(j));
}

// Inner node i of the radix tree over n >= 2 sorted codes: it covers [first, last] and splits after
// `split` (left child [first, split], right child [split + 1, last]). A child that covers more than one
// code is inner node `split` (left) or `split + 1` (right).
struct LbvhRange { int32_t first, last, split; };
RT_LBVH_HD LbvhRange lbvh_node(const uint32_t *codes, int32_t n, int32_t i) {
    const int d = lbvh_delta(codes, n, i, int64_t(i) + 1) - lbvh_delta(codes, n, i, int64_t(i) - 1) < 0 ? -1 : 1;
    const int dmin = lbvh_delta(codes, n, i, int64_t(i) - d);
    int64_t lmax = 2;
    while (lbvh_delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = lbvh_delta(codes, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (lbvh_delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    LbvhRange r;
    r.first = static_cast<int32_t>(d > 0 ? i : j);
    r.last = static_cast<int32_t>(d > 0 ? j : i);
    r.split = static_cast<int32_t>(i + s * d + (d < 0 ? -1 : 0));
    return r;
}

}  // namespace rt
