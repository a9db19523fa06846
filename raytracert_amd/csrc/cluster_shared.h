// cluster_shared.h — the definitions of the agglomerative builder (RT_BUILD_CLUSTER; parallel locally-
// ordered clustering, Meister & Bittner 2018) that the host statement (bvh.cpp build_cluster) and the
// kernels (rt_kernels.hip k_cluster_*) must perform identically: both include this text. Only IEEE
// binary64 + - *, float compares and integer operations are used (both sides are compiled without
// contraction).
#pragma once

#include <cstdint>

#include "lbvh_shared.h"
#include "rt_internal.h"   // RT_BVH_MAX_LEAF and the leaf ref layout (kBvhLeafBit, kBvhCountShift)

namespace rt {

constexpr int kClusterRadius = 8;       // r: a cluster looks at the r positions on each side of its own
// The iteration budget: twice the largest count measured (DESIGN.md "GPU BVH build: RT_BUILD_CLUSTER"),
// the margin for deformed meshes. A build that ends the budget with more than one cluster falls back.
constexpr int kClusterMaxIters = 106;
// At or below this many clusters one workgroup finishes the remaining iterations in LDS (k_cluster_tail): the
// last thousand clusters take some twenty iterations, which would be four small launches each.
constexpr int kClusterTail = 1024;
// The host reads the cluster count back after every this many iterations of a device build and stops
// queueing at the tail's size (0: the whole budget is queued blind). Chosen by measurement, DESIGN.md.
constexpr int kClusterReadbackEvery = 8;

// One cluster: a child ref (a leaf ref, or the creation index of a binary node: leaf bit clear) and the
// exact min / max union of the padded boxes below it.
struct ClusterBox { float lo[3], hi[3]; };

// Union in argument order (Box::grow: std::min / std::max as the compares they are, so signed zeros and
// equal bounds resolve the same way on both sides).
RT_LBVH_HD ClusterBox cluster_union(const ClusterBox &a, const ClusterBox &b) {
    ClusterBox u;
    for (int k = 0; k < 3; ++k) {
        u.lo[k] = (b.lo[k] < a.lo[k]) ? b.lo[k] : a.lo[k];
        u.hi[k] = (a.hi[k] < b.hi[k]) ? b.hi[k] : a.hi[k];
    }
    return u;
}

// The distance of two clusters: the half-area of their union box, in binary64 from the binary32 bounds
// (no overflow for extents near FLT_MAX, no inf * 0). A NaN (bounds that are not finite) counts as +inf, so
// the key below stays a total order.
RT_LBVH_HD double cluster_distance(const ClusterBox &a, const ClusterBox &b) {
    const ClusterBox u = cluster_union(a, b);
    const double dx = double(u.hi[0]) - double(u.lo[0]);
    const double dy = double(u.hi[1]) - double(u.lo[1]);
    const double dz = double(u.hi[2]) - double(u.lo[2]);
    const double d = (dx * dy + dy * dz) + dz * dx;
    return d == d ? d : __builtin_inf();
}

// Nearest neighbour of position i among c clusters: the j != i with |i - j| <= kClusterRadius that
// minimises (distance, i XOR j), compared lexicographically; -1 when there is none (c == 1). The key is
// symmetric in i and j and unique per i, so the globally smallest pair is mutual: every iteration merges.
// box(j) returns the box of position j (global memory on the host, the LDS stage in the kernel).
template <typename BoxAt>
RT_LBVH_HD int32_t cluster_nearest(int32_t i, int32_t c, BoxAt box) {
    const int32_t b = i - kClusterRadius > 0 ? i - kClusterRadius : 0;
    const int32_t e = i + kClusterRadius < c - 1 ? i + kClusterRadius : c - 1;
    const ClusterBox me = box(i);
    int32_t best = -1;
    double bd = 0;
    uint32_t bx = 0;
    for (int32_t j = b; j <= e; ++j) {
        if (j == i) continue;
        const double d = cluster_distance(me, box(j));
        const uint32_t x = static_cast<uint32_t>(i) ^ static_cast<uint32_t>(j);
        if (best < 0 || d < bd || (d == bd && x < bx)) { best = j; bd = d; bx = x; }
    }
    return best;
}

// What position i does this iteration, given the nearest neighbours: 0 it survives unchanged, 1 it is
// the lower position of a mutual pair and keeps the slot as the merged cluster, 2 it is the higher
// position and dies. nn is range-checked by the caller.
RT_LBVH_HD int cluster_role(int32_t i, int32_t j, int32_t nn_of_j) {
    if (j < 0 || nn_of_j != i) return 0;
    return i < j ? 1 : 2;
}

// A merge of two single-triangle leaves in adjacent leaf slots makes one two-triangle leaf, not a node.
RT_LBVH_HD bool cluster_leaf_pair(uint32_t ref_lo, uint32_t ref_hi, uint32_t *merged) {
    if (RT_BVH_MAX_LEAF < 2) return false;
    const uint32_t one = kBvhLeafBit | (1u << kBvhCountShift), mask = (1u << kBvhCountShift) - 1u;
    if ((ref_lo & ~mask) != one || (ref_hi & ~mask) != one) return false;
    if ((ref_hi & mask) != (ref_lo & mask) + 1u) return false;
    *merged = kBvhLeafBit | (2u << kBvhCountShift) | (ref_lo & mask);
    return true;
}

}  // namespace rt
