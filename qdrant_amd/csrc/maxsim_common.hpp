// maxsim_common.hpp — what the fused MaxSim kernels (maxsim_fused.hip: f32 rows, maxsim_f16.hip: f16 rows, maxsim_u8.hip: u8 rows) share on the
// device: the LDS-DMA copy of a row piece, the LDS-only barrier, a block's run of the row stream, the piece swizzle of the 16-byte operand reads, the
// constants of the tile meta and the scratch tile.
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

// The block's run [b0, b1) of the row stream [s0, s0 + total): the candidates whose start S[c] falls in the block's equal share of it.  A point is
// never shared between blocks; b0 >= b1: nothing to do.
struct MsfRun {
    uint64_t b0, b1;
};
__device__ __forceinline__ MsfRun msf_block_run(const uint64_t *S, const uint32_t *cmap, uint64_t s0, uint64_t total) {
    const uint64_t end = s0 + total;
    const uint64_t share = (total + gridDim.x - 1) / gridDim.x;
    auto first_start_from = [&](uint64_t x) -> uint64_t {       // the smallest candidate start >= x that has rows behind it (or the stream's end)
        if (x >= end) return end;
        const uint32_t c = cmap[x - s0];
        return S[c] == x ? x : S[(uint64_t)c + 1];
    };
    const uint64_t lo = s0 + (uint64_t)blockIdx.x * share;
    return MsfRun{first_start_from(lo), first_start_from(lo + share)};
}

// The piece swizzle of the kernels whose A operand is one ds_read_b128 per lane (f16, u8): piece e of tile row m sits in slot
// m (pieces per row) + (e ^ (msf_swz16(m & 15) & mask)), mask = the low bits that stay inside the row.  A ds_read_b128 is served sixteen lanes at a
// time - {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 - i.e. two k-groups kq, kq + 1 with complementary rows; the swizzle makes their
// sixteen slots distinct mod 16 (the 64 banks): bits 0-1 = {0, 2, 3, 1}[m >> 2] (with kq: four values per m & 3), bit 2 = bit 1 of m, bit 3 = bit 0
// of m.  A row of 4 (2 j + 1) pieces spreads m & 3 itself (mask 3), one of 8 (2 j + 1) pieces m & 1 (mask 7), one of 2 (2 j + 1) pieces all of
// m & 7 and the two k-groups by parity (mask 0).
__device__ __forceinline__ uint32_t msf_swz16(uint32_t m) { return ((0x78u >> (2u * ((m >> 2) & 3u))) & 3u) | ((m & 2u) << 1) | ((m & 1u) << 3); }
constexpr uint32_t msf_swz16_mask(int pieces_per_row) { return pieces_per_row % 4 ? 0u : pieces_per_row % 8 ? 3u : pieces_per_row % 16 ? 7u : 15u; }

}  // namespace qmx
