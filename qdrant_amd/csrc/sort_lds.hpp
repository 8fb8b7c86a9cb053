// sort_lds.hpp — the in-LDS key sort the one-work-group-per-request kernels share (fusion.hip, formula.hip).
#pragma once
#include "common.hpp"

namespace qmx {

// ascending bitonic sort of n (a power of two >= 2) keys in LDS by the whole work-group of BLOCK lanes
template <int BLOCK>
__device__ __forceinline__ void bitonic_sort_lds(uint64_t *keys, uint32_t n) {
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < n; i += BLOCK) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint64_t a = keys[i], b = keys[x];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace qmx
