// okx_philox.hpp — the counter-based generator of the ensemble passes (kernel units only): Philox4x32-10, what the sampler
// (okx_sample.hip) draws latents and stratum keys from and the bootstrap (okx_bootstrap.hip) its weights.  The counter's
// last word carries the purpose (OKX_SAMPLE_PURPOSE_*, include/okx.h) in bits 8-15, so the passes never share a draw.
// Integers only; open_kinematics_amd/ensemble_sample.py (philox4x32_10) is the NumPy definition.
#pragma once

#include <hip/hip_runtime.h>

namespace okx {
namespace rng {

__device__ inline void philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0, unsigned int k1,
                                     unsigned int* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace rng
}  // namespace okx
