// dark_lights.h — which lights cannot reach a hit (RT_TUNE_DARK_LIGHTS): the rule chain_step applies
// before it walks a light's shadow ray. A light is dark for a hit when shade_hit's diffuse and specular
// terms for it are both exactly zero whatever isShadow says AND the in-place normalisations an unshadowed
// light makes (raytracing.cpp:199,213) leave the hit's normal as it is, bit for bit, so the verdict can
// change neither the colour nor the reflection ray. Such a light is marked shadowed without a walk.
// Header-only and host-callable, so tests/cxx/dark_lights_check.cpp checks the same code on the CPU
// (built with -ffp-contract=off, as the kernels are).
//
// Why the margin suffices (m = kDarkMargin = 1e-3, u = 2^-24; every vector below is the float vector
// shade_hit itself makes):
//  * A normal n0 that passes dark_fixed_point is the output of Vec3D::normalize (or has a squared length
//    that rounds to 0, and then no compare below can pass), so 0.7 < |n0| < 1.3 even when the squared
//    length was subnormal; the lights' lnorm are outputs of the same function: |lnorm| < 1.3, or 0, or NaN.
//  * Diffuse: shade_hit takes max(dot(N(n0), lnorm), 0). N(n0) = r n0 (1 + e) per component with
//    r = 1 / |n0| in (0.7, 1.5) and |e| <= u, so dot(N(n0), lnorm) <= r dot(n0, lnorm) + 4 u |n0| |lnorm|
//    <= -0.7 m + 1e-6 < 0 when the float dot(n0, lnorm) <= -m (its own rounding error is < 4 u 1.7).
//  * Specular: with `normal` back at n0 (the fixed point), shade_hit takes max(dot(H, n0), 0),
//    H = N(N(cam - P) + N(L - P)). dark_facing(n0, v) means dot(n0, v) <= -m |v| + 6e-7 |v| (the float
//    dot's error is < 4 u |n0| |v|, the squares' a few u relative), so
//    dot(n0, N(v)) <= -m + 1e-6 for both v, their float sum S has dot(n0, S) <= -2 m + 3e-6, hence
//    |S| >= 1.5e-3: S is far from 0 (two opposite unit vectors cannot both face away from n0 by the
//    margin: dot(n0, V) <= -m and V + L ~ 0 give dot(n0, L) >= m - 1e-6), its squared length is a normal
//    float, H = S / |S| (1 + 2 u) with |S| <= 2.001, and dot(H, n0) <= (-2 m + 3e-6) / 2.001 + 1e-6 < 0.
//  * Both maxima are then +0; Kd * 0, Ks * spec_pow(+0, Ns) with Ns > 0 finite, and their products with
//    Tr are signed zeros (finite material, dark_material_ok), and adding a signed zero to a colour that
//    is never -0 (it starts at +0 and +0 + -0 = +0) leaves its bits.
// No NaN passes: every compare is written so that a NaN operand makes it false.
#ifndef RT_DARK_LIGHTS_H_
#define RT_DARK_LIGHTS_H_

#include <cmath>
#include <cstdint>
#include <cstring>

#include "spec_pow.h"   // RT_HD

namespace rt {

constexpr float kDarkMargin = 1e-3f;

// Vec3D::normalize (Vec3D.h:142-151), the kernels' normalize(V3 &).
RT_HD inline void normalize3(float &x, float &y, float &z) {
    const float len = sqrtf(x * x + y * y + z * z);
    if (len == 0.0f) return;
    const float rez = 1.0f / len;
    x *= rez; y *= rez; z *= rez;
}

RT_HD inline uint32_t dark_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, f);
#else
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
#endif
}

// dot(n, l) <= -m for a unit l (a light's lnorm): the first, cheapest test of a light.
RT_HD inline bool dark_light_side(const float n[3], const float l[3]) {
    return n[0] * l[0] + n[1] * l[1] + n[2] * l[2] <= -kDarkMargin;
}

// dot(n, v) <= -m |v| on squared quantities (no square root). A product that overflowed or fell
// below 1e-30 decides nothing (tt >= 1e-30 with tt >= m^2 vv also makes vv a normal float or 0).
RT_HD inline bool dark_facing(const float n[3], const float v[3]) {
    const float t = n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
    const float vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const float tt = t * t;
    return t < 0.0f && tt >= (kDarkMargin * kDarkMargin) * vv && tt >= 1e-30f && tt < INFINITY;
}

// The specular compares of light L for the hit at P seen from cam: both the view vector and the
// light vector face away from n by the margin (shade_hit's own cam - P and L - P).
RT_HD inline bool dark_view(const float n[3], const float P[3], const float cam[3]) {
    const float v[3] = {cam[0] - P[0], cam[1] - P[1], cam[2] - P[2]};
    return dark_facing(n, v);
}
RT_HD inline bool dark_spec_light(const float n[3], const float P[3], const float L[3]) {
    const float v[3] = {L[0] - P[0], L[1] - P[1], L[2] - P[2]};
    return dark_facing(n, v);
}

// N^c(n) == n bit for bit, c = the normalize(normal) calls of one unshadowed light (0, 1 or 2).
RT_HD inline bool dark_fixed_point(const float n[3], int c) {
    float x = n[0], y = n[1], z = n[2];
    for (int i = 0; i < c; ++i) normalize3(x, y, z);
    return dark_bits(x) == dark_bits(n[0]) && dark_bits(y) == dark_bits(n[1]) && dark_bits(z) == dark_bits(n[2]);
}

// The material's part, decided once at upload (kMatDarkOk in DevMaterial::flags): every factor a zero
// term is multiplied by is finite, and a specular material's exponent makes spec_pow(+0, Ns) = +0.
RT_HD inline bool dark_material_ok(const float Kd[3], const float Ks[3], float Tr, float Ns, bool has_spec) {
    const float big = 3.4028234663852886e38f;   // FLT_MAX: |x| <= big is false for inf and NaN
    bool ok = fabsf(Tr) <= big;
    for (int k = 0; k < 3; ++k) ok = ok && fabsf(Kd[k]) <= big && fabsf(Ks[k]) <= big;
    if (has_spec) ok = ok && Ns > 0.0f && Ns <= big;
    return ok;
}

// The whole rule for one light (the host check and the tests; the kernels run the same pieces in
// cost order over all lights of a hit): diffuse / spec = the terms shade_hit evaluates for this hit.
RT_HD inline bool dark_light(const float n[3], const float P[3], const float cam[3], const float L[3], const float lnorm[3],
                             bool diffuse, bool spec) {
    if (!dark_light_side(n, lnorm)) return false;
    if (spec && !(dark_view(n, P, cam) && dark_spec_light(n, P, L))) return false;
    return dark_fixed_point(n, (diffuse ? 1 : 0) + (spec ? 1 : 0));
}

}  // namespace rt

#endif  // RT_DARK_LIGHTS_H_
