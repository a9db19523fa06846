// Host check of the dark-light rule's margin (raytracert_amd/csrc/dark_lights.h): the same header the
// kernels use, built with g++ -ffp-contract=off. For random and adversarial (normal, P, cam, light) tuples,
// whenever the rule says dark, the binary32 values shade_hit would compute (raytracing.cpp:197-232 in the
// kernels' operation order) are exact zeros for both terms, their dot products are negative, and the
// normal after the light's normalisations is the stored normal bit for bit.
// Prints "ok <tuples> <dark> <dark near the margin>" and returns 0, or the first failures and 1.
// Usage: dark_lights_check [random tuples, default 10000000]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "dark_lights.h"

namespace {

float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }   // Vec3D.h:192-194
float max_std(float a, float b) { return (a < b) ? b : a; }

long long n_all = 0, n_dark = 0, n_near = 0, n_bad = 0;

// One tuple through the rule and, when it says dark, through shade_hit's arithmetic for one unshadowed light.
void check(const float n0[3], const float P[3], const float cam[3], const float L[3], bool diffuse, bool spec, float Ns) {
    ++n_all;
    float lnorm[3] = {L[0], L[1], L[2]};
    rt::normalize3(lnorm[0], lnorm[1], lnorm[2]);   // shade_params
    if (!rt::dark_light(n0, P, cam, L, lnorm, diffuse, spec)) return;
    ++n_dark;
    float normal[3] = {n0[0], n0[1], n0[2]};
    bool bad = false;
    float d = -1.0f, s = -1.0f;
    if (diffuse) {
        rt::normalize3(normal[0], normal[1], normal[2]);
        d = dot3(normal, lnorm);
        const float term = 0.75f * max_std(d, 0.0f);
        bad = bad || !(d < 0.0f) || rt::dark_bits(term) != 0u;
    }
    if (spec) {
        float V[3] = {cam[0] - P[0], cam[1] - P[1], cam[2] - P[2]};
        rt::normalize3(V[0], V[1], V[2]);
        rt::normalize3(normal[0], normal[1], normal[2]);
        float Lv[3] = {L[0] - P[0], L[1] - P[1], L[2] - P[2]};
        rt::normalize3(Lv[0], Lv[1], Lv[2]);
        float H[3] = {V[0] + Lv[0], V[1] + Lv[1], V[2] + Lv[2]};
        rt::normalize3(H[0], H[1], H[2]);
        s = dot3(H, normal);
        const float term = 0.5f * rt::spec_pow(max_std(s, 0.0f), Ns);
        bad = bad || !(s < 0.0f) || rt::dark_bits(term) != 0u;
    }
    for (int k = 0; k < 3; ++k) bad = bad || rt::dark_bits(normal[k]) != rt::dark_bits(n0[k]);
    if ((diffuse && d > -4e-3f) || (spec && s > -4e-3f)) ++n_near;
    if (bad && n_bad++ < 10)
        std::printf("BAD n0 %a %a %a P %a %a %a cam %a %a %a L %a %a %a diffuse %d spec %d: d %a s %a normal %a %a %a\n", n0[0], n0[1],
                    n0[2], P[0], P[1], P[2], cam[0], cam[1], cam[2], L[0], L[1], L[2], diffuse, spec, d, s, normal[0], normal[1], normal[2]);
}

void check_modes(const float n0[3], const float P[3], const float cam[3], const float L[3], float Ns) {
    check(n0, P, cam, L, true, true, Ns);
    check(n0, P, cam, L, true, false, Ns);
    check(n0, P, cam, L, false, true, Ns);
}

}  // namespace

int main(int argc, char **argv) {
    const long long n_random = argc > 1 ? std::atoll(argv[1]) : 10000000;
    std::mt19937_64 r(7);
    std::normal_distribution<float> g(0.0f, 1.0f);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    auto unit = [&](float v[3], int rounds) {   // a stored normal: normalised `rounds` times (0: raw)
        v[0] = g(r); v[1] = g(r); v[2] = g(r);
        if (r() % 8 == 0) v[r() % 3] = 0.0f;    // axis-aligned and planar normals
        for (int i = 0; i < rounds; ++i) rt::normalize3(v[0], v[1], v[2]);
    };
    // random tuples: points and lights in a box a few units wide around the origin, as the scenes are
    for (long long i = 0; i < n_random; ++i) {
        float n0[3], P[3], cam[3], L[3];
        unit(n0, static_cast<int>(r() % 4));
        for (int k = 0; k < 3; ++k) { P[k] = 2.0f * u(r); cam[k] = 5.0f * u(r); L[k] = 5.0f * u(r); }
        const float Ns = 1.0f + 100.0f * std::fabs(u(r));
        check(n0, P, cam, L, r() % 4 != 0, r() % 4 != 1, Ns);
    }
    // adversarial tuples: the light and the camera placed so that the facing cosines sit within a few
    // parts in 1e3 of the margin on either side, V + L nearly zero, tiny and huge distances, tiny normals
    const float scales[] = {1e-18f, 1e-12f, 1e-6f, 1e-3f, 1.0f, 1e3f, 1e6f, 1e12f, 1e18f, 3e19f};
    for (int i = 0; i < 400000; ++i) {
        float n0[3], t[3], P[3], cam[3], L[3];
        unit(n0, 1 + static_cast<int>(r() % 3));
        unit(t, 1);
        const float tn = dot3(t, n0);
        for (int k = 0; k < 3; ++k) t[k] -= tn * n0[k];   // a tangent direction
        rt::normalize3(t[0], t[1], t[2]);
        const float c1 = -rt::kDarkMargin * (1.0f + 4e-3f * u(r)), c2 = -rt::kDarkMargin * (1.0f + 4e-3f * u(r));
        const float s1 = scales[r() % 10], s2 = scales[r() % 10];
        const bool origin = r() % 2;
        const bool opposite = r() % 4 == 0;   // the light opposite the camera: V + L ~ 0
        for (int k = 0; k < 3; ++k) {
            P[k] = origin ? 0.0f : u(r);
            cam[k] = P[k] + s1 * (c1 * n0[k] + t[k]);
            L[k] = P[k] + s2 * (c2 * n0[k] + (opposite ? -t[k] : t[k]));
        }
        check_modes(n0, P, cam, L, 1.0f + static_cast<float>(r() % 64));
        if (i % 16 == 0) {   // normals whose squared length is subnormal or rounds to zero
            const float tiny = std::ldexp(1.0f, -60 - static_cast<int>(r() % 20));
            float nt[3] = {n0[0] * tiny, n0[1] * tiny, n0[2] * tiny};
            check_modes(nt, P, cam, L, 10.0f);
        }
    }
    if (n_bad) { std::printf("FAILED %lld of %lld dark tuples\n", n_bad, n_dark); return 1; }
    std::printf("ok %lld %lld %lld\n", n_all, n_dark, n_near);
    return 0;
}
