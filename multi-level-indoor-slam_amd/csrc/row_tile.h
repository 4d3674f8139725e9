// The bf16 operand tile of the fused row-tile kernels (lg_ffn.hip, mixvpr.hip): 64 rows of
// 512 bf16 (1 KiB) in LDS, XOR-swizzled 16-B chunks, and the epilogue write into it.
#pragma once
#include "common.h"

constexpr int ROWB = 1024;  // LDS bytes per tile row: 512 bf16

// 16-B chunk c of row r at slot c ^ (r & 15): the 16 lanes of each ds_read_b128 lane
// group (rows {0-3,12-15,20-27} + 32 k, one chunk) then hit 16 distinct bank quads.
__device__ __forceinline__ int cat_off(int row, int chunk) { return row * ROWB + ((chunk ^ (row & 15)) << 4); }

// Epilogue writes into [x | msg] / the GELU tile: lanes l and
// l + 32 hold the two 8-B halves of one 16-B chunk (rows col and 32 + col in m-tiles 0 / 1);
// a v_permlane32_swap gives lane l < 32 m-tile 0's whole chunk and lane l + 32 m-tile 1's,
// written as one b128.  LDS writes retire 128 B per cycle in lane order (b128: 8 lanes,
// banks modulo 128 B; profiles/r05x_lds_calibration.txt): 8 consecutive rows at slots
// chunk ^ (r & 15) are distinct modulo 128 B -- the per-half b64 writes paid 2-way.
__device__ __forceinline__ void cat_pair_write(char* lds, int chunk, uint2 m0v, uint2 m1v) {
    const int lane = threadIdx.x & 63, col = lane & 31, hh = lane >> 5;
    const auto s0 = __builtin_amdgcn_permlane32_swap(m0v.x, m1v.x, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(m0v.y, m1v.y, false, false);
    *reinterpret_cast<uint4*>(lds + cat_off(32 * hh + col, chunk)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
}

__device__ __forceinline__ bf16x8 ld16(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
