// maxsim_common.hpp — what the fused MaxSim kernels (maxsim_fused.hip: f32 rows, maxsim_f16.hip: f16 rows) share on the device: the LDS-DMA copy of
// a row piece, the LDS-only barrier, the constants of the tile meta and the scratch tile.
#pragma once
#include "kernels.hpp"

namespace qmx {

typedef __attribute__((address_space(3))) unsigned char msf_lds_byte;

// 64 16-byte pieces (per-lane source) -> LDS at the wave-uniform byte address lds_dst + 16 lane.  Invisible to the compiler's s_waitcnt
// bookkeeping on purpose: the tile loop counts these loads itself (the compiler's own loads only make its counts stricter).
__device__ __forceinline__ void msf_glds16(const unsigned char *src, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}

// the block's barrier for LDS traffic alone: no vmcnt(0), which would drain the row stream
__device__ __forceinline__ void msf_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

constexpr uint32_t MSF_NONE = 0xFFFFFFFFu;      // cmap / tile meta: no candidate (rows past the block's stream)
constexpr int MSF_SIM_P = 68;                   // pitch of the scratch tile in floats: rows 4 k + j of a D register land 16 banks apart

}  // namespace qmx
