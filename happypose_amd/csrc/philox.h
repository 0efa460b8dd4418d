// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the one device copy of the generator behind
// every seeded draw of the library: multipliers 0xD2511F53 / 0xCD9E8D57, key schedule += 0x9E3779B9 / 0xBB67AE85, ten rounds.  Its
// Python restatement is tests/mesh_sample_ref.py.
//
// Counter and key layout belong to the caller: each feature documents its own (row lo, row hi, call, 0), (index, image, stream, 0),
// ... and the seed's two halves as the key, and results that repeat from a seed depend on those staying as they are.
//
// Integer arithmetic only.  Shared headers are compiled OUTSIDE the `#pragma clang fp contract(off)` of the files that include
// them, so nothing with a contractible floating-point expression (a bare a * b + c) may be added here.
#pragma once

#include "common.h"

namespace hp {

namespace philox_detail {
__device__ __forceinline__ void philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
}
}  // namespace philox_detail

// c <- the four output words of counter c under key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_detail::philox_round(c, k0, k1);
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

}  // namespace hp
