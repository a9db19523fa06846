// oracle/spec_pow_twin.cpp — TEST INFRASTRUCTURE ONLY.
//
// The host build of the kernels' specular power (raytracert_amd/csrc/spec_pow.h), compiled by g++ with
// -O2 -ffp-contract=off: the same source the device compiles, so a colour the oracle makes with it
// (ora_set_spec_pow(1)) is what the kernels must give bit for bit, and a direct comparison of the two
// builds (tests/test_gpu_device_math.py) says whether hipcc's device code rounds every operation of the
// header as the host does.
#include "../raytracert_amd/csrc/spec_pow.h"

#include <cstdint>

extern "C" float ora_spec_pow_twin(float x, float y) { return rt::spec_pow(x, y); }

// The same over arrays (a million ctypes calls take seconds; this takes milliseconds).
extern "C" void ora_spec_pow_twin_batch(const float *x, const float *y, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = rt::spec_pow(x[i], y[i]);
}
