// LightGlue block projections (upstream SelfBlock.Wqkv + rotary encoding, CrossBlock
// to_qk / to_v; LightGlue(features='superpoint') as called by
// LightGlue._detect_and_match_native, scripts/semantic_gating/geometric_verification.py:
// 263-312) over the flat token layout, writing the attention operands directly:
//   Q, K  bf16 [4 heads][Npad][64]                 (self: q, k rotated; cross: qk)
//   V^T   bf16 [4][Npad / 64][64 d][64 keys]       (attention.hip's tiled V^T)
// Rows outside live segments are written as zeros.
//
// One workgroup = 8 waves walks 64-token tiles of one 256-column part (q, k or v) of the
// projection; the bf16 x tile [64][256] sits in LDS (XOR-swizzled 16-B chunks: chunk c of
// row r at slot c ^ (r & 15), so the 16 lanes of a ds_read_b128 lane group hit 16 distinct
// bank quads), the weights are packed k-step-major [16][N][16].  Wave w owns output columns
// 32 w .. +32 of the part for both 32-token m-tiles.  The q / k parts compute
// C^T = W . X^T, which hands a lane 4 consecutive head dims of one token (the rotary
// pairs are lane-local); the v part swaps the MFMA operands, C = X . W^T, which hands a
// lane 4 consecutive tokens of one dim, the layout of a transposed V^T row.  Same
// fragments, operand order only.
//
// The forms that lost are in the history, not here: one workgroup per 64- or 128-token
// tile with the weights streamed from L2 (128-token tiles 2-7 % slower, self 2.39 vs 2.35 ms,
// cross 1.27 vs 1.19 ms at 2 M tokens, tools/archive/gpu_ab_ffn_proj.sh: the weight stream
// is not what bounds the kernel), the weights-resident form with a serial epilogue
// (profiles/r02f_ab_proj_resident.txt; 82.2 vs 63.0 ms per 2048-pair call against the
// pipelined form below, identical Q / K / V^T hashes, profiles/r04z_ab_proj_pipe.txt),
// and its timing probes (profiles/r02p_ab_proj_factor_swizzle.txt, r04an_proj_pipe_probes.txt).
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int ROWB = 512;  // LDS bytes per token row: 256 bf16

__device__ __forceinline__ bf16x8 ld16(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

// a tile's rotary factors: 16 KiB, [16 pairs][64 rows] float4 (common.h lg_fac4); a lane
// reads the float4 of its row for one frequency pair: the 32 lanes of a half-wave read 512
// contiguous bytes, one conflict-free ds_read_b128 (the [64][32] cos / sin images before
// round 5 took two ds_read_b64 with 2-way conflicts, profiles/r05c_lds_conflict_calibration.txt)
__device__ __forceinline__ float4 fac_tile(const float* fc, int r, int p) {
    return *reinterpret_cast<const float4*>(fc + ((p * 64 + r) << 2));
}

// ---------------------------------------------------------------- weights-resident form
// One workgroup (8 waves) per (part, slot) walks token tiles; wave w keeps its 32
// output columns' weights for all 16 k-steps in registers (64 VGPRs, loaded once), so
// the GEMM reads only the x tile from LDS and nothing from L2.  The next tile's x rows
// arrive by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, XOR swizzle
// applied to the source addresses) into another buffer while this tile is computed and
// written.  Grid: per XCD `slots` x NPART workgroups; the parts of one
// token tile run on one XCD at the same time (tile t -> XCD t % 8), so x is read from
// HBM once and from that XCD's L2 by the other parts.
typedef __attribute__((address_space(3))) char lds_char;
__device__ __forceinline__ unsigned lds_addr(char* p) { return (unsigned)(uintptr_t)(lds_char*)p; }
// The `s_nop 0` is the SALU-write-M0 -> LDS-DMA-read-M0 wait state (gfx9 family): hipcc
// sets M0 for the "{m0}" operand with an s_mov_b32 placed directly in front of the
// statement and pads hazards only for instructions it models, not for asm.  Without it
// the DMA could take the previous piece's M0 and land 1 KiB in the wrong slot, depending
// on issue timing (run-to-run / co-scheduling dependent results: DESIGN.md §5, r03a).
__device__ __forceinline__ void dma16(const void* g, unsigned m0) {
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "{m0}"(m0) : "memory");
}

// ---------------------------------------------------------------- pipelined epilogue
// The epilogue of tile t - 1 is issued INSIDE the GEMM of tile t:
// every wave's bias / rotary / mask / bf16 staging of the previous tile's accumulators is
// cut into 8 slices (4 column groups x 2 m-tiles), one after every second k-step, so the
// VALU work fills the MFMA gaps instead of running in a phase of its own (the serial form
// spends about as long in its epilogue as in its GEMM).  Three LDS buffers: tile t's x
// rows (GEMM), tile t - 1's staging image over its dead x rows (+ its factors / live
// bytes), tile t + 1's DMA.  Only the copy-out stays a phase of its own, after the
// staging barrier.  Results are those of the serial-epilogue form bit for bit (same
// accumulators, same epilogue arithmetic).
// Paired staging: lanes l and l + 32 hold the two 8-B halves of one 16-B
// chunk (q / k: head dims 8c..+3 and 8c+4..+7 of token r; v: tokens 8g..+3 and 8g+4..+7 of
// dim d).  slice_*_val packs a slice's 8 B; stage_pair takes the m-tile 0 and 1 halves,
// swaps lanes 32-63 of the first with lanes 0-31 of the second (v_permlane32_swap), so
// lane l < 32 holds m-tile 0's whole chunk and lane l + 32 m-tile 1's, and writes it as
// ONE ds_write_b128 into an image whose chunk c of row r sits at slot c ^ (r & 7).  LDS
// writes retire 128 B per cycle in lane order (b128: 8 lanes, bank = address mod 128 B),
// reads 256 B (b128: 16 lanes, mod 256 B): the 8 consecutive rows of a write group then
// hit 8 distinct 16-B slots mod 128, and the copy-out's b128 reads of 2 rows x 8 chunks 16
// distinct slots mod 256 -- both conflict-free (tools/lds_probe.hip, profiles/
// r05x_lds_calibration.txt; a (r >> 1) & 7 swizzle paid 2-way on every write, per-half
// b64 writes 4 conflict cycles each: -1.4 % for the pair writes, profiles/
// r05u_ab_proj_staging.txt, conflict share 0.39 -> 0.0 and -1.6 % for this swizzle,
// profiles/r05ab_ab_proj_pair_swizzle.txt).
// Staging image over a dead x tile: [4 heads][64 rows][64] bf16.  Rows are tokens for q / k
// and head dims for V^T; either way a head's 64 rows are ONE contiguous 8 KiB block of the
// destination, written as whole 1 KiB pieces.
__device__ __forceinline__ int stage_pair_off(int h, int row, int c) {
    return (h * 64 + row) * 128 + ((c ^ (row & 7)) << 4);
}
__device__ __forceinline__ void stage_pair(uint2 m0v, uint2 m1v, char* lds, int h, int row, int c) {
    const auto s0 = __builtin_amdgcn_permlane32_swap(m0v.x, m1v.x, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(m0v.y, m1v.y, false, false);
    *reinterpret_cast<uint4*>(lds + stage_pair_off(h, row, c)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
}

template <bool SELF>
__device__ __forceinline__ uint2 slice_qk_val(int g, int mt, const f32x16& a, const float* bias_l, const float* fc,
                                              const uint8_t* live_l) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hh = lane >> 5;
    const int n = 32 * wave + 8 * g + 4 * hh;
    const float4 b = *reinterpret_cast<const float4*>(bias_l + n);
    const int r = 32 * mt + col;
    float x0 = a[4 * g] + b.x, x1 = a[4 * g + 1] + b.y, x2 = a[4 * g + 2] + b.z, x3 = a[4 * g + 3] + b.w;
    if (SELF) {  // t * cos + rotate_half(t) * sin, uncontracted as torch
        const float4 cs = fac_tile(fc, r, (n & 63) >> 2);  // cos j, cos j + 1, sin j, sin j + 1
        const float r0 = __fadd_rn(__fmul_rn(x0, cs.x), __fmul_rn(-x1, cs.z));
        const float r1 = __fadd_rn(__fmul_rn(x1, cs.x), __fmul_rn(x0, cs.z));
        const float r2 = __fadd_rn(__fmul_rn(x2, cs.y), __fmul_rn(-x3, cs.w));
        const float r3 = __fadd_rn(__fmul_rn(x3, cs.y), __fmul_rn(x2, cs.w));
        x0 = r0; x1 = r1; x2 = r2; x3 = r3;
    }
    // branch-free mask: a branch here would end the basic block and with it the
    // scheduler's freedom to interleave this slice with the GEMM's MFMAs
    const uint32_t keep = 0u - (uint32_t)(live_l[r] != 0);
    return make_uint2(pack_bf16x2(x0, x1) & keep, pack_bf16x2(x2, x3) & keep);
}
// q / k pair write of column group g: row 32 hh + col, chunk (32 wave + 8 g) / 8 of head h
__device__ __forceinline__ void stage_pair_qk(int g, uint2 m0v, uint2 m1v, char* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hh = lane >> 5;
    const int n = 32 * wave + 8 * g;
    stage_pair(m0v, m1v, lds, n >> 6, 32 * hh + col, (n & 63) >> 3);
}

__device__ __forceinline__ uint2 slice_v_val(int g, int mt, const f32x16& a, const float* bias_l,
                                             const uint8_t* live_l) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hh = lane >> 5;
    const float b = bias_l[32 * wave + col];
    const int r = 32 * mt + 8 * g + 4 * hh;
    const uint32_t lv = *reinterpret_cast<const uint32_t*>(live_l + r);
    const float v0 = (lv & 0xff) ? a[4 * g] + b : 0.f;
    const float v1 = (lv & 0xff00) ? a[4 * g + 1] + b : 0.f;
    const float v2 = (lv & 0xff0000) ? a[4 * g + 2] + b : 0.f;
    const float v3 = (lv >> 24) ? a[4 * g + 3] + b : 0.f;
    return make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
}
// V^T pair write of token group g: row d, chunk g + 4 hh (tokens 32 hh + 8 g ..) of head h
__device__ __forceinline__ void stage_pair_v(int g, uint2 m0v, uint2 m1v, char* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hh = lane >> 5;
    const int n = 32 * wave + col;
    stage_pair(m0v, m1v, lds, n >> 6, n & 63, g + 4 * hh);
}

// acc_new = GEMM of the x tile in `xl`; with STAGE, slice i of the previous tile's
// staging (acc_old into `sl`) after k-step 2 i.
template <bool SELF, bool IS_V, bool STAGE>
__device__ __forceinline__ void pipe_gemm(const bf16x8 (&wf)[16], const char* xl, f32x16 (&acc)[2],
                                          const f32x16 (&old)[2], char* sl, const float* bias_l, const float* fc,
                                          const uint8_t* live_l) {
    const int lane = threadIdx.x & 63, col = lane & 31, hh = lane >> 5;
    const char* xrow = xl + col * ROWB;
    const int sw = col & 15;
    bf16x8 xa[2], xb[2];
    uint2 pend = make_uint2(0u, 0u);  // m-tile 0's half of the pending pair
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) xa[mt] = *reinterpret_cast<const bf16x8*>(xrow + 32 * mt * ROWB + ((hh ^ sw) << 4));
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        bf16x8(&cur)[2] = (ks & 1) ? xb : xa;
        bf16x8(&nxt)[2] = (ks & 1) ? xa : xb;
        if (ks < 15) {
            const int cn = ((2 * (ks + 1) + hh) ^ sw) << 4;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) nxt[mt] = *reinterpret_cast<const bf16x8*>(xrow + 32 * mt * ROWB + cn);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            acc[mt] = IS_V ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[mt], wf[ks], acc[mt], 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], cur[mt], acc[mt], 0, 0, 0);
        if (STAGE && !(ks & 1)) {  // m-tile 0's half at ks = 4 g, the pair write at 4 g + 2
            const int g = ks >> 2, mt = (ks >> 1) & 1;
            const uint2 v = IS_V ? slice_v_val(g, mt, old[mt], bias_l, live_l)
                                 : slice_qk_val<SELF>(g, mt, old[mt], bias_l, fc, live_l);
            if (mt == 0) {
                pend = v;
            } else if (IS_V) {
                stage_pair_v(g, pend, v, sl);
            } else {
                stage_pair_qk(g, pend, v, sl);
            }
        }
    }
}

// copy-out of a staged 64-token tile: per head one contiguous [64 rows][64] block at
// (h * Npad + m0) * 64 (for V^T the tiled [64 d][64 keys] block of the tile's keys)
__device__ __forceinline__ void copy_out64(bool is_v, int part, int m0, const char* lds, bf16_t* __restrict__ Q,
                                           bf16_t* __restrict__ K, bf16_t* __restrict__ Vt, int Npad) {
    bf16_t* dst = is_v ? Vt : (part == 0 ? Q : K);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int L = p * 512 + threadIdx.x, h = L / 512, row = (L >> 3) & 63, c = L & 7;
        *reinterpret_cast<uint4*>(dst + ((size_t)h * Npad + m0 + row) * 64 + c * 8) =
            *reinterpret_cast<const uint4*>(lds + stage_pair_off(h, row, c));
    }
}

template <bool SELF, bool IS_V>
__device__ __forceinline__ void pipe_tiles(const bf16x8 (&wf)[16], char* ring, const float* bias_l,
                                           const bf16_t* __restrict__ xcopy, int ldx, const float* __restrict__ efac,
                                           const uint8_t* __restrict__ live,
                                           bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ Vt,
                                           int Npad, int part, int t0, int stride, int ntiles) {
    constexpr int R = 64, XB = R * ROWB, BUF = XB + (SELF ? 2 * R * 32 * 4 : 0), SLOT = BUF + 256;
    auto bufs = [&](int i) { return ring + i * SLOT; };
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int drow = 8 * wave + (lane >> 5), dslot = lane & 31;
    auto issue = [&](int tile, char* buf) {
        const unsigned base = lds_addr(buf) + 4096 * wave;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = drow + 2 * i;
            dma16(xcopy + (size_t)(tile * R + row) * ldx + ((dslot ^ (row & 15)) * 8), base + 1024 * i);
        }
        if (SELF) {  // the tile's 16 KiB factor block: two 1 KiB pieces per wave
#pragma unroll
            for (int i = 0; i < 2; ++i)
                dma16(efac + (size_t)tile * (R * 64) + (2 * wave + i) * 256 + 4 * lane,
                      lds_addr(buf) + XB + 1024 * (2 * wave + i));
        }
        if (wave == 0 && lane < R / 16) dma16(live + (size_t)tile * R + 16 * lane, lds_addr(buf) + BUF);
    };
    f32x16 acc0[2], acc1[2];  // the GEMM's and the staged tile's, alternating (compile-time roles)
    issue(t0, bufs(0));
    int t = t0, tp = -1, it = 0;  // tile in the GEMM, tile being staged (-1: none)
    // one iteration; PAR = it & 1 picks the accumulator roles
    auto step = [&](f32x16 (&an)[2], const f32x16 (&ao)[2]) -> bool {
        const int bx = it % 3, bp = (it + 2) % 3, bn = (it + 1) % 3;
        // tile t's DMA has landed (only the previous iteration's 4 copy-out stores per lane
        // were issued after it; none in the first two iterations)
        if (it < 2) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        else __builtin_amdgcn_s_waitcnt(0x0F74);         // vmcnt(4)
        __syncthreads();  // every wave's DMA; every wave's copy-out reads of buffer bn
        const int tn = t + stride;
        if (tn < ntiles) issue(tn, bufs(bn));
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) an[mt][i] = 0.f;
        char* sl = bufs(bp);
        const float* fc = reinterpret_cast<const float*>(sl + XB);
        if (tp >= 0) {
            pipe_gemm<SELF, IS_V, true>(wf, bufs(bx), an, ao, sl, bias_l, fc,
                                        reinterpret_cast<const uint8_t*>(sl + BUF));
            __syncthreads();  // staging written
            copy_out64(IS_V, part, tp * R, sl, Q, K, Vt, Npad);
        } else {
            pipe_gemm<SELF, IS_V, false>(wf, bufs(bx), an, ao, sl, bias_l, fc,
                                         reinterpret_cast<const uint8_t*>(sl + BUF));
        }
        tp = t;
        ++it;
        if (tn >= ntiles) {  // the last tile: its staging alone
            __syncthreads();  // every wave has read its x rows
            char* sx = bufs(bx);
            const float* fx = reinterpret_cast<const float*>(sx + XB);
            const uint8_t* lx = reinterpret_cast<const uint8_t*>(sx + BUF);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (IS_V)
                    stage_pair_v(g, slice_v_val(g, 0, an[0], bias_l, lx), slice_v_val(g, 1, an[1], bias_l, lx), sx);
                else
                    stage_pair_qk(g, slice_qk_val<SELF>(g, 0, an[0], bias_l, fx, lx),
                                  slice_qk_val<SELF>(g, 1, an[1], bias_l, fx, lx), sx);
            }
            __syncthreads();
            copy_out64(IS_V, part, tp * R, sx, Q, K, Vt, Npad);
            return true;
        }
        t = tn;
        return false;
    };
    for (;;) {
        if (step(acc0, acc1)) return;
        if (step(acc1, acc0)) return;
    }
}

template <bool SELF>
__global__ __launch_bounds__(512) void k_lg_proj_pipe(const bf16_t* __restrict__ xcopy, int ldx,
                                                        const bf16_t* __restrict__ W, const float* __restrict__ bias,
                                                        const float* __restrict__ efac,
                                                        const uint8_t* __restrict__ live, bf16_t* __restrict__ Q,
                                                        bf16_t* __restrict__ K, bf16_t* __restrict__ Vt, int Npad,
                                                        int slots) {
    constexpr int N = SELF ? 768 : 512, NPART = SELF ? 3 : 2, R = 64;
    constexpr int SLOT = R * ROWB + (SELF ? 2 * R * 32 * 4 : 0) + 256;  // x, factors, live bytes (pipe_tiles)
    __shared__ __attribute__((aligned(16))) char ring[3 * SLOT];
    __shared__ __attribute__((aligned(16))) float bias_l[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hh = lane >> 5;
    const int xcd = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
    const int part = j % NPART, slot = j / NPART;
    const int ntiles = Npad / R, stride = 8 * slots;
    const int t0 = xcd + 8 * slot;
    if (slot >= slots || t0 >= ntiles) return;
    if (threadIdx.x < 256) bias_l[threadIdx.x] = bias[256 * part + threadIdx.x];  // read after the loop-top barrier
    bf16x8 wf[16];
    {
        const bf16_t* wrow = W + (size_t)(256 * part + 32 * wave + col) * 16 + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) wf[ks] = ld16(wrow + (size_t)ks * N * 16);
    }
    if (part == NPART - 1)
        pipe_tiles<SELF, true>(wf, ring, bias_l, xcopy, ldx, efac, live, Q, K, Vt, Npad, part, t0, stride, ntiles);
    else
        pipe_tiles<SELF, false>(wf, ring, bias_l, xcopy, ldx, efac, live, Q, K, Vt, Npad, part, t0, stride,
                                ntiles);
}

}  // namespace

int mlg_lg_proj(bool self_block, const bf16_t* xcopy, int ldx, const bf16_t* W, const float* bias, const float* efac,
                const uint8_t* live, bf16_t* Q, bf16_t* K, bf16_t* Vt, int Npad, hipStream_t s) {
    if (Npad <= 0 || (Npad % 64) || ldx < 256 || (ldx % 8)) return MLG_EINVAL;
    static const int cus = [] {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 8)
            return 256;
        return c;
    }();
    const int npart = self_block ? 3 : 2, ntiles = Npad / 64;
    // one workgroup per CU (256 VGPRs, 64-96 KiB LDS), `slots` part-groups per XCD
    const int slots = std::max(1, std::min((cus / 8) / npart, (ntiles + 7) / 8));
    const unsigned grid = (unsigned)(8 * slots * npart);
    if (self_block)
        hipLaunchKernelGGL(k_lg_proj_pipe<true>, dim3(grid), dim3(512), 0, s, xcopy, ldx, W, bias, efac, live, Q, K, Vt,
                           Npad, slots);
    else
        hipLaunchKernelGGL(k_lg_proj_pipe<false>, dim3(grid), dim3(512), 0, s, xcopy, ldx, W, bias,
                           (const float*)nullptr, live, Q, (bf16_t*)nullptr, Vt, Npad, slots);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
