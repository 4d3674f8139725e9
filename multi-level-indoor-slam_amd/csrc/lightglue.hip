// LightGlue matcher for a batch of keyframe pairs (gfx950).
//
// Restates LightGlue(features='superpoint') as called by the reference
// (geometric_verification.py:224-233, 285-305; semantics in oracle/lightglue.py).
// All images of all pairs live in ONE flat token layout: segment 2p (image a of pair
// p) and 2p+1 (image b), each padded to a multiple of 64 rows.  Per layer the shared
// weights run as single GEMMs over every token (gemm_bf16.hip, bf16 MFMA, f32
// accumulation); attention is one ragged launch (attention.hip k_attention_varlen)
// whose tasks are the self (seg -> seg) or cross (a -> b, b -> a) pairings.
// State: x f32 [Npad, 256] (residual stream) and cat bf16 [Npad, 512] = [x | message]
// so the FFN's torch.cat([x, message]) is free.  After each layer but the last the
// token confidences and matchability give per-segment statistics; the host reads them
// (one small D2H copy per layer), stops pairs whose confident ratio exceeds
// depth_confidence (their assignment runs at that layer), prunes segments above the
// pruning threshold, and compacts the layout with one gather.
// The host side of that -- segment layout, attention task tables, layer 0's frame layout,
// the per-layer stop / prune / compaction decision -- is pair_plan.h; this file validates,
// carves the workspace, uploads the plan's tables and launches.
#include <vector>

#include "common.h"
#include "kernels.h"
#include "pair_plan.h"
#include "ws_carve.h"
#include "../../include/mlgate.h"

namespace {

using pair_plan::Seg;
static_assert(sizeof(pair_plan::Task) == sizeof(int4) && sizeof(pair_plan::Move) == sizeof(int4),
              "the host tables are uploaded by bytes into the kernels' int4 tables");

constexpr int LG_D = 256, LG_H = 4, LG_L = 9;

// ------------------------------------------------------------------ init
// normalize_keypoints without image_size: size = 1 + max - min per image,
// k' = (k - size / 2) / (max(size) / 2).  One workgroup per segment -> norm[seg] =
// (shift_x, shift_y, scale).
__global__ __launch_bounds__(256) void k_lg_kpnorm(const Seg* __restrict__ segs, const float* __restrict__ kpts,
                                                   int kmax, float4* __restrict__ norm) {
    const Seg sg = segs[blockIdx.x];
    const int tid = threadIdx.x;
    const float* kp = kpts + (size_t)sg.frame * kmax * 2;
    __shared__ float red[4][256];
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (int i = tid; i < sg.len; i += 256) {
        mnx = fminf(mnx, kp[2 * i]);
        mxx = fmaxf(mxx, kp[2 * i]);
        mny = fminf(mny, kp[2 * i + 1]);
        mxy = fmaxf(mxy, kp[2 * i + 1]);
    }
    red[0][tid] = mnx;
    red[1][tid] = mny;
    red[2][tid] = mxx;
    red[3][tid] = mxy;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] = fminf(red[0][tid], red[0][tid + o]);
            red[1][tid] = fminf(red[1][tid], red[1][tid + o]);
            red[2][tid] = fmaxf(red[2][tid], red[2][tid + o]);
            red[3][tid] = fmaxf(red[3][tid], red[3][tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float sx = 1.f + red[2][0] - red[0][0], sy = 1.f + red[3][0] - red[1][0];
        norm[blockIdx.x] = make_float4(sx / 2.f, sy / 2.f, fmaxf(sx, sy) / 2.f, 0.f);
    }
}

// 64 rows of one segment per workgroup: Fourier positional encoding (cos / sin of
// Wr . k', 32 frequencies), x = desc, cat[:, :256] = bf16(desc), ind = source index;
// rows past len zeroed.  With mv (layer 0's self block already run per frame): the live
// rows' x and bf16 copy come from that block's output instead, mv[seg] = (pair offset,
// live rows, frame offset, -) -- no separate row-gather pass (+0.3 %, same counts,
// profiles/r04x_ab_lg_init_fused.txt).
__global__ __launch_bounds__(256) void k_lg_init(const Seg* __restrict__ segs, const float4* __restrict__ norm,
                                                 const float* __restrict__ kpts, const float* __restrict__ desc,
                                                 int kmax, const float* __restrict__ Wr, float* __restrict__ x,
                                                 bf16_t* __restrict__ cat, float4* __restrict__ efac,
                                                 int32_t* __restrict__ ind,
                                                 const int4* __restrict__ mv = nullptr,
                                                 const float* __restrict__ xf = nullptr,
                                                 const bf16_t* __restrict__ catf = nullptr) {
    const Seg sg = segs[blockIdx.y];
    const int r0 = blockIdx.x * 64;
    if (r0 >= ((sg.len + 63) & ~63)) return;
    const float4 nm = norm[blockIdx.y];
    const float* kp = kpts + (size_t)sg.frame * kmax * 2;
    const float* ds = desc + (size_t)sg.frame * kmax * LG_D;
    for (int e = threadIdx.x; e < 64 * 16; e += 256) {
        const int i = r0 + e / 16, p = e % 16;
        const size_t r = (size_t)sg.off + i;
        const bool live = i < sg.len;
        float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);  // cos f, cos f + 1, sin f, sin f + 1
        if (live) {
            const float kx = (kp[2 * i] - nm.x) / nm.z, ky = (kp[2 * i + 1] - nm.y) / nm.z;
            const float p0 = kx * Wr[4 * p] + ky * Wr[4 * p + 1];
            const float p1 = kx * Wr[4 * p + 2] + ky * Wr[4 * p + 3];
            cs = make_float4(cosf(p0), cosf(p1), sinf(p0), sinf(p1));
        }
        efac[lg_fac4(r, p)] = cs;
        if (p == 0) ind[r] = live ? i : -1;
    }
    if (mv) {
        const size_t fo = (size_t)mv[blockIdx.y].z;
        for (int e = threadIdx.x; e < 64 * LG_D / 4; e += 256) {
            const int i = r0 + e / (LG_D / 4), c4 = (e % (LG_D / 4)) * 4;
            const size_t r = (size_t)sg.off + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            uint2 o = make_uint2(0u, 0u);
            if (i < sg.len) {
                v = *reinterpret_cast<const float4*>(xf + (fo + i) * LG_D + c4);
                o = *reinterpret_cast<const uint2*>(catf + (fo + i) * 512 + c4);
            }
            *reinterpret_cast<float4*>(x + r * LG_D + c4) = v;
            *reinterpret_cast<uint2*>(cat + r * 512 + c4) = o;
        }
        return;
    }
    for (int e = threadIdx.x; e < 64 * LG_D / 4; e += 256) {
        const int i = r0 + e / (LG_D / 4), c4 = (e % (LG_D / 4)) * 4;
        const size_t r = (size_t)sg.off + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < sg.len) v = *reinterpret_cast<const float4*>(ds + (size_t)i * LG_D + c4);
        *reinterpret_cast<float4*>(x + r * LG_D + c4) = v;
        uint2 o;
        o.x = pack_bf16x2(v.x, v.y);
        o.y = pack_bf16x2(v.z, v.w);
        *reinterpret_cast<uint2*>(cat + r * 512 + c4) = o;
    }
}

// ------------------------------------------------------------------ confidences
// Token confidence / matchability heads run inside the cross block's fused tail
// (lg_ffn.hip, mlg_lg_conf_i): flags[r] = (conf < thr) | keep << 1, lz = logsigmoid(z).
// stats[seg] = {#(conf < thr), #keep}: one workgroup per segment
__global__ __launch_bounds__(256) void k_lg_segstats(const Seg* __restrict__ segs, const uint8_t* __restrict__ flags,
                                                     int* __restrict__ stats) {
    const Seg sg = segs[blockIdx.x];
    int low = 0, kp = 0;
    for (int i = threadIdx.x; i < sg.len; i += 256) {
        const uint8_t f = flags[sg.off + i];
        low += f & 1;
        kp += f >> 1;
    }
    low = wave_sum((float)low) + 0.5f;  // exact for counts < 2^24
    kp = wave_sum((float)kp) + 0.5f;
    __shared__ int sh[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[0][wave] = low; sh[1][wave] = kp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[2 * blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        stats[2 * blockIdx.x + 1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    }
}

// ------------------------------------------------------------------ compaction
// new row dst_off + rank(i) <- old row src_off + i for tokens with keep (or all when
// keep_all): x, cat[:, :256], enc, ind.  One workgroup per (old) segment.
__global__ __launch_bounds__(256) void k_lg_compact(const int4* __restrict__ moves, const uint8_t* __restrict__ keep,
                                                    const float* __restrict__ x, const float4* __restrict__ efac,
                                                    const int32_t* __restrict__ ind,
                                                    float* __restrict__ x2, bf16_t* __restrict__ cat2,
                                                    float4* __restrict__ efac2,
                                                    int32_t* __restrict__ ind2) {
    const int4 mv = moves[blockIdx.x];  // src_off, src_len, dst_off, keep_all
    __shared__ int rank[2048 + 64];
    __shared__ int wsum[4];
    const int tid = threadIdx.x;
    // ordered ranks: 256 threads x contiguous chunks
    const int per = (mv.y + 255) / 256;
    const int a0 = tid * per, a1 = min(mv.y, a0 + per);
    int c = 0;
    for (int i = a0; i < a1; ++i) c += mv.w ? 1 : (keep[mv.x + i] >> 1);
    // block exclusive scan of c
    int v = c;
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    int r = base + v - c;
    for (int i = a0; i < a1; ++i) rank[i] = (mv.w || (keep[mv.x + i] >> 1)) ? r++ : -1;
    const int newlen = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    const int padded = (newlen + 63) & ~63;
    // 16-B x loads / stores and 8-B bf16 stores per lane (the same RNE conversion per
    // element as f32_to_bf16); a wave moves one whole 1 KiB row of x per instruction
    for (int e = tid; e < mv.y * (LG_D / 4); e += 256) {
        const int i = e / (LG_D / 4), c4 = (e % (LG_D / 4)) * 4;
        const int rk = rank[i];
        if (rk < 0) continue;
        const float4 val = *reinterpret_cast<const float4*>(x + (size_t)(mv.x + i) * LG_D + c4);
        *reinterpret_cast<float4*>(x2 + (size_t)(mv.z + rk) * LG_D + c4) = val;
        *reinterpret_cast<uint2*>(cat2 + (size_t)(mv.z + rk) * 512 + c4) =
            make_uint2(pack_bf16x2(val.x, val.y), pack_bf16x2(val.z, val.w));
    }
    for (int e = tid; e < mv.y * 16; e += 256) {
        const int i = e / 16, p = e % 16;
        const int rk = rank[i];
        if (rk < 0) continue;
        efac2[lg_fac4((size_t)(mv.z + rk), p)] = efac[lg_fac4((size_t)(mv.x + i), p)];
    }
    for (int i = tid; i < mv.y; i += 256)
        if (rank[i] >= 0) ind2[mv.z + rank[i]] = ind[mv.x + i];
    // zero the padding rows of the new segment
    for (int e = tid; e < (padded - newlen) * (LG_D / 4); e += 256) {
        const int i = newlen + e / (LG_D / 4), c4 = (e % (LG_D / 4)) * 4;
        *reinterpret_cast<float4*>(x2 + (size_t)(mv.z + i) * LG_D + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<uint2*>(cat2 + (size_t)(mv.z + i) * 512 + c4) = make_uint2(0u, 0u);
    }
    for (int e = tid; e < (padded - newlen) * 16; e += 256) {
        const int i = newlen + e / 16, p = e % 16;
        efac2[lg_fac4((size_t)(mv.z + i), p)] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = newlen + tid; i < padded; i += 256) ind2[mv.z + i] = -1;
}

// ------------------------------------------------------------------ assignment
// For every finishing pair a (table entry Asg): S = final_proj(x0) . final_proj(x1)^T
// (the two 1/4 scales applied here as one exact 1/16), the row / column log_softmax
// terms (torch form (x - max) - log(sum exp(x - max))), and the row / column argmax of
// (s0 + s1) + (lz0 + lz1)  (first index on ties, as torch.max), then the mutual filter.
// Row / column statistics are indexed by layout row, so all pairs share the buffers.
// Tile grids carry the pair in blockIdx.z, line grids in blockIdx.y.
//
//   k_asg_sim      128 x 128 GEMM tile -> S (whole float4 rows) + the tile's partial
//                  (max, sum exp) of every row and column, from the LDS-staged tile;
//   k_asg_stats    combines the partials -> row / column (max, log sum exp);
//   k_asg_arg      reads each 64 x 128 tile of S once -> per-tile best (score, index)
//                  of every row and column;
//   k_asg_argfinal combines them -> row argmax + value, column argmax.
// S is written once and read once.
struct Asg {
    int m, n, ra, rb;  // rows of image a / b, their first layout rows
    long soff;         // S offset (floats)
    int pair, ld;      // pair index, S row stride (n rounded up to 4: float4 rows)
    int lo_first, pad; // image a's frame index > image b's: k_asg_sim's cross-term order
};

constexpr int SBM = 128;               // k_asg_sim tile (rows = columns)
constexpr int TSS = SBM + 4;           // its LDS row stride: the 16 lanes of a b128 group (16 rows)
                                       // and the 64 lanes of a b32 column read hit distinct banks
constexpr int ARM = 64, ARN = 128;     // k_asg_arg tile
constexpr int TSA = ARN + 8;           // its LDS row stride: b128 groups of 8 rows x 2 halves
// Both kernels scan full tiles straight-line and leave the edge tiles to the general loops:
// k_asg_arg -19 %, k_asg_sim -1.5 %, digest identical (profiles/r05ah_ab_assignment_full_tiles.txt).

// per-tile partials: part[((slot * 2 + dir) * tiles + t) * kmax + i]; dir 0 = rows
// (t = 128-column tile), dir 1 = columns (t = row tile: 128 rows in k_asg_sim's
// statistics, 64 in k_asg_arg's bests)
__device__ __forceinline__ size_t part_at(int slot, int dir, int t, int i, int kmax) {
    return ((size_t)(slot * 2 + dir) * ((kmax + ARM - 1) / ARM) + t) * kmax + i;
}

// S = MD[ra .. ra + m) . MD[rb .. rb + n)^T of every listed pair in ONE launch.  MD is
// final_proj(x) (f32 accumulate) held as bf16 hi + lo halves (hi = bf16(y), lo =
// bf16(y - hi), k-step-major [16][rows][16]; gemm_bf16.hip EpiBiasSplitBF16), and the
// product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 with f32 accumulation:
// operand error ~2^-17, dropped lo.lo ~2^-18 relative -- f32-class accuracy (upstream
// runs this einsum in float32) at 3 bf16 MFMAs instead of 8 exact-f32 32x32x2 ones per
// 16-deep k-step.  4 waves of 64 x 64; each wave streams its operand fragments straight
// from L2 (one contiguous 1 KiB per wave-load), double-buffered one k-step ahead.
#ifndef ASG_PF
#define ASG_PF 1
#endif
__global__ __launch_bounds__(256, 2) void k_asg_sim(const Asg* __restrict__ tab, const bf16_t* __restrict__ MDH,
                                                    const bf16_t* __restrict__ MDL, int rows,
                                                    float* __restrict__ Sall, float2* __restrict__ part, int kmax) {
    const Asg a = tab[blockIdx.z];
    const int m0 = blockIdx.y * SBM, n0 = blockIdx.x * SBM;
    if (m0 >= a.m || n0 >= a.n) return;
    __shared__ __attribute__((aligned(16))) float T[SBM * TSS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const size_t step = (size_t)rows * 16;
    size_t ao[2], bo[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        ao[x] = (size_t)(a.ra + min(m0 + wm * 64 + 32 * x + col, a.m - 1)) * 16 + 8 * hh;
        bo[x] = (size_t)(a.rb + min(n0 + wn * 64 + 32 * x + col, a.n - 1)) * 16 + 8 * hh;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
    // ASG_PF k-steps of fragments in flight (2 = double buffer); each step's 8 loads are
    // L2 round trips that one step of 12 MFMAs does not cover
    constexpr int NB = ASG_PF + 1;
    bf16x8 ah[NB][2], al[NB][2], bh[NB][2], bl[NB][2];  // [buffer][x or y]
#pragma unroll
    for (int pf = 0; pf < ASG_PF; ++pf) {
        const size_t o = (size_t)pf * step;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            ah[pf][x] = *reinterpret_cast<const bf16x8*>(MDH + o + ao[x]);
            al[pf][x] = *reinterpret_cast<const bf16x8*>(MDL + o + ao[x]);
            bh[pf][x] = *reinterpret_cast<const bf16x8*>(MDH + o + bo[x]);
            bl[pf][x] = *reinterpret_cast<const bf16x8*>(MDL + o + bo[x]);
        }
    }
#pragma unroll
    for (int ks = 0; ks < LG_D / 16; ++ks) {
        const int cb = ks % NB, nb = (ks + ASG_PF) % NB;
        if (ks + ASG_PF < LG_D / 16) {
            const size_t o = (size_t)(ks + ASG_PF) * step;
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                ah[nb][x] = *reinterpret_cast<const bf16x8*>(MDH + o + ao[x]);
                al[nb][x] = *reinterpret_cast<const bf16x8*>(MDL + o + ao[x]);
                bh[nb][x] = *reinterpret_cast<const bf16x8*>(MDH + o + bo[x]);
                bl[nb][x] = *reinterpret_cast<const bf16x8*>(MDL + o + bo[x]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // next step's loads stay ahead of this step's MFMAs
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                // the two cross terms in a canonical order: hi of the lower frame's image x lo
                // of the other first, whichever side it is on.  The swapped call (b, a) then
                // adds the same products in the same order to every element, so S(b, a) is
                // S(a, b)^T bit for bit and LightGlue(b, a) is exactly swap(LightGlue(a, b))
                // -- what lets the full gate match each unordered pair once (pipeline.py).
                // (A fixed ah.bl-then-al.bh order rounded the swapped call's cross terms the
                // other way round: 1 of 1024 reverse pairs kept a different match, r02k.)
                if (!a.lo_first) {
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[cb][x], bl[cb][y], acc[x][y], 0, 0, 0);
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[cb][x], bh[cb][y], acc[x][y], 0, 0, 0);
                } else {
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[cb][x], bh[cb][y], acc[x][y], 0, 0, 0);
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[cb][x], bl[cb][y], acc[x][y], 0, 0, 0);
                }
                acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[cb][x], bh[cb][y], acc[x][y], 0, 0, 0);
            }
    }
    // D[i][j]: col j = lane & 31, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int j = wn * 64 + y * 32 + col;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                T[(wm * 64 + x * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * TSS + j] = acc[x][y][r];
        }
    __syncthreads();
    const int mr = min(SBM, a.m - m0), nc = min(SBM, a.n - n0);
    float* S = Sall + a.soff;
#pragma unroll 4
    for (int it = 0; it < SBM / 8; ++it) {
        // ld is a multiple of 4 and columns n .. ld are scratch: whole float4s while c < nc
        const int r = it * 8 + (tid >> 5), c = (tid & 31) * 4;
        if (r < mr && c < nc)
            *reinterpret_cast<float4*>(S + (size_t)(m0 + r) * a.ld + n0 + c) =
                *reinterpret_cast<const float4*>(T + r * TSS + c);
    }
    // partial softmax statistics: threads 0-127 one row each, 128-255 one column each;
    // exp(v / 16 - mx) as exp2 of one FMA (v_exp_f32)
    constexpr float L2E = 1.4426950408889634f;
    const bool colw = tid >= SBM;
    const int q = tid & (SBM - 1);
    if (q >= (colw ? nc : mr)) return;
    float mx = -INFINITY, sm = 0.f;
    if ((colw ? mr : nc) == SBM) {
        // full-length line: straight-line scans, no per-element bounds test (same order)
        if (colw) {
#pragma unroll 8
            for (int e = 0; e < SBM; ++e) mx = fmaxf(mx, T[e * TSS + q]);
            mx *= 0.0625f;
            const float nm = -mx * L2E;
#pragma unroll 8
            for (int e = 0; e < SBM; ++e) sm += __builtin_amdgcn_exp2f(fmaf(T[e * TSS + q], 0.0625f * L2E, nm));
        } else {
            const float* p = T + q * TSS;
#pragma unroll 8
            for (int e = 0; e < SBM; e += 4) {
                const float4 v = *reinterpret_cast<const float4*>(p + e);
                mx = fmaxf(mx, v.x);
                mx = fmaxf(mx, v.y);
                mx = fmaxf(mx, v.z);
                mx = fmaxf(mx, v.w);
            }
            mx *= 0.0625f;
            const float nm = -mx * L2E;
#pragma unroll 8
            for (int e = 0; e < SBM; e += 4) {
                const float4 v = *reinterpret_cast<const float4*>(p + e);
                sm += __builtin_amdgcn_exp2f(fmaf(v.x, 0.0625f * L2E, nm));
                sm += __builtin_amdgcn_exp2f(fmaf(v.y, 0.0625f * L2E, nm));
                sm += __builtin_amdgcn_exp2f(fmaf(v.z, 0.0625f * L2E, nm));
                sm += __builtin_amdgcn_exp2f(fmaf(v.w, 0.0625f * L2E, nm));
            }
        }
    } else if (colw) {
        for (int e = 0; e < mr; ++e) mx = fmaxf(mx, T[e * TSS + q]);
        mx *= 0.0625f;
        const float nm = -mx * L2E;
        for (int e = 0; e < mr; ++e) sm += __builtin_amdgcn_exp2f(fmaf(T[e * TSS + q], 0.0625f * L2E, nm));
    } else {
        const float* p = T + q * TSS;
        for (int e = 0; e < nc; e += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + e);
            mx = fmaxf(mx, v.x);
            if (e + 1 < nc) mx = fmaxf(mx, v.y);
            if (e + 2 < nc) mx = fmaxf(mx, v.z);
            if (e + 3 < nc) mx = fmaxf(mx, v.w);
        }
        mx *= 0.0625f;
        const float nm = -mx * L2E;
        for (int e = 0; e < nc; e += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + e);
            sm += __builtin_amdgcn_exp2f(fmaf(v.x, 0.0625f * L2E, nm));
            if (e + 1 < nc) sm += __builtin_amdgcn_exp2f(fmaf(v.y, 0.0625f * L2E, nm));
            if (e + 2 < nc) sm += __builtin_amdgcn_exp2f(fmaf(v.z, 0.0625f * L2E, nm));
            if (e + 3 < nc) sm += __builtin_amdgcn_exp2f(fmaf(v.w, 0.0625f * L2E, nm));
        }
    }
    part[colw ? part_at(blockIdx.z, 1, blockIdx.y, n0 + q, kmax) : part_at(blockIdx.z, 0, blockIdx.x, m0 + q, kmax)] =
        make_float2(mx, sm);
}

// row / column (max, log sum exp) from k_asg_sim's partials; grid (.., pairs, 2 dirs)
__global__ __launch_bounds__(256) void k_asg_stats(const Asg* __restrict__ tab, const float2* __restrict__ part,
                                                   int kmax, float* __restrict__ rmax, float* __restrict__ rlog,
                                                   float* __restrict__ cmax, float* __restrict__ clog) {
    const Asg a = tab[blockIdx.y];
    const int dir = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (dir ? a.n : a.m)) return;
    const int nt = ((dir ? a.m : a.n) + SBM - 1) / SBM;
    const float2* p = part + part_at(blockIdx.y, dir, 0, i, kmax);
    float M = -INFINITY;
    for (int t = 0; t < nt; ++t) M = fmaxf(M, p[(size_t)t * kmax].x);
    float S = 0.f;
    for (int t = 0; t < nt; ++t) S += p[(size_t)t * kmax].y * expf(p[(size_t)t * kmax].x - M);
    const int o = dir ? a.rb + i : a.ra + i;
    (dir ? cmax : rmax)[o] = M;
    (dir ? clog : rlog)[o] = logf(S);
}

__device__ __forceinline__ float lg_score(float v, float rm, float rl, float cm, float cl, float cert) {
    return (((v - rm) - rl) + ((v - cm) - cl)) + cert;
}

// (score, index) a beats b: higher score, the lower index on ties
__device__ __forceinline__ bool beats(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// per-tile best (score, index) of every row and column of a 64 x 128 tile of S (4 tiles
// in flight per CU so the HBM read of one overlaps the scoring of another): threads
// 0-127 two per row (alternate float4 column chunks, combined by one shuffle), 128-255
// one per column; each scans increasing indices with strict >, keeping the first index
__global__ __launch_bounds__(256, 4) void k_asg_arg(const Asg* __restrict__ tab, const float* __restrict__ Sall,
                                                    const float* __restrict__ rmax, const float* __restrict__ rlog,
                                                    const float* __restrict__ cmax, const float* __restrict__ clog,
                                                    const float* __restrict__ lz, float2* __restrict__ part, int kmax) {
    const Asg a = tab[blockIdx.z];
    const int m0 = blockIdx.y * ARM, n0 = blockIdx.x * ARN;
    if (m0 >= a.m || n0 >= a.n) return;
    __shared__ __attribute__((aligned(16))) float T[ARM * TSA];
    __shared__ float4 sr[ARM], sc[ARN];  // (max, log sum, log-sigmoid) of the tile's rows / columns
    const int tid = threadIdx.x;
    const int mr = min(ARM, a.m - m0), nc = min(ARN, a.n - n0);
    const float* S = Sall + a.soff;
#pragma unroll
    for (int it = 0; it < ARM / 8; ++it) {
        const int r = it * 8 + (tid >> 5), c = (tid & 31) * 4;
        if (r < mr && c < nc)
            *reinterpret_cast<float4*>(T + r * TSA + c) =
                *reinterpret_cast<const float4*>(S + (size_t)(m0 + r) * a.ld + n0 + c);
    }
    if (tid < ARM) {
        if (tid < mr) {
            const int o = a.ra + m0 + tid;
            sr[tid] = make_float4(rmax[o], rlog[o], lz[o], 0.f);
        }
    } else if (tid >= ARN) {
        const int j = tid - ARN;
        if (j < nc) {
            const int o = a.rb + n0 + j;
            sc[j] = make_float4(cmax[o], clog[o], lz[o], 0.f);
        }
    }
    __syncthreads();
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (tid < ARN) {
        const int r = tid >> 1, h = tid & 1;
        if (r < mr && nc == ARN) {
            // full-width tile: straight-line scan, no per-element bounds test (same scores,
            // same order, same strict > -- the general loop below, branch-free)
            const float4 me = sr[r];
            const float* p = T + r * TSA;
#pragma unroll 4
            for (int q = 0; q < ARN / 8; ++q) {
                const int c = 8 * q + 4 * h;
                const float4 v = *reinterpret_cast<const float4*>(p + c);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 ot = sc[c + k];
                    const float s = lg_score(vv[k] * 0.0625f, me.x, me.y, ot.x, ot.y, me.z + ot.z);
                    const bool g = s > best;
                    best = g ? s : best;
                    bi = g ? c + k : bi;
                }
            }
        } else if (r < mr) {
            const float4 me = sr[r];
            const float* p = T + r * TSA;
            for (int c = 4 * h; c < nc; c += 8) {
                const float4 v = *reinterpret_cast<const float4*>(p + c);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (c + k >= nc) break;
                    const float4 ot = sc[c + k];
                    const float s = lg_score(vv[k] * 0.0625f, me.x, me.y, ot.x, ot.y, me.z + ot.z);
                    if (s > best) {
                        best = s;
                        bi = c + k;
                    }
                }
            }
        }
        const float ob = __shfl_xor(best, 1, 64);
        const int oi = __shfl_xor(bi, 1, 64);
        if (beats(ob, oi, best, bi)) {
            best = ob;
            bi = oi;
        }
        if (h == 0 && r < mr)
            part[part_at(blockIdx.z, 0, blockIdx.x, m0 + r, kmax)] =
                make_float2(best, __int_as_float(bi == 0x7fffffff ? bi : n0 + bi));
    } else {
        const int j = tid - ARN;
        if (j >= nc) return;
        const float4 me = sc[j];
        if (mr == ARM) {
#pragma unroll 8
            for (int e = 0; e < ARM; ++e) {
                const float4 ot = sr[e];
                const float s = lg_score(T[e * TSA + j] * 0.0625f, ot.x, ot.y, me.x, me.y, ot.z + me.z);
                const bool g = s > best;
                best = g ? s : best;
                bi = g ? e : bi;
            }
        } else {
            for (int e = 0; e < mr; ++e) {
                const float4 ot = sr[e];
                const float s = lg_score(T[e * TSA + j] * 0.0625f, ot.x, ot.y, me.x, me.y, ot.z + me.z);
                if (s > best) {
                    best = s;
                    bi = e;
                }
            }
        }
        part[part_at(blockIdx.z, 1, blockIdx.y, n0 + j, kmax)] =
            make_float2(best, __int_as_float(bi == 0x7fffffff ? bi : m0 + bi));
    }
}

// row argmax + value, column argmax from the per-tile bests (tiles in increasing index
// order, strict >: the first index on ties); grid (.., pairs, 2 dirs).  A line with no
// finite score (NaN input) points at index 0 with value -inf.
__global__ __launch_bounds__(256) void k_asg_argfinal(const Asg* __restrict__ tab, const float2* __restrict__ part,
                                                      int kmax, int* __restrict__ arg, float* __restrict__ val) {
    const Asg a = tab[blockIdx.y];
    const int dir = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (dir ? a.n : a.m)) return;
    const int nt = dir ? (a.m + ARM - 1) / ARM : (a.n + ARN - 1) / ARN;
    const float2* p = part + part_at(blockIdx.y, dir, 0, i, kmax);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int t = 0; t < nt; ++t) {
        const float2 c = p[(size_t)t * kmax];
        if (c.x > best) {
            best = c.x;
            bi = __float_as_int(c.y);
        }
    }
    if (bi == 0x7fffffff) {
        bi = 0;
        best = -INFINITY;
    }
    if (dir) {
        arg[a.rb + i] = bi;
    } else {
        arg[a.ra + i] = bi;
        val[a.ra + i] = best;
    }
}

// mutual nearest + exp(score) > th -> matches (ind0[i], ind1[m0[i]]) in row order.
// One workgroup per finishing pair.
__global__ __launch_bounds__(256) void k_lg_filter(const Asg* __restrict__ tab, const int* __restrict__ arg,
                                                   const float* __restrict__ val, const int32_t* __restrict__ ind,
                                                   float th, int kmax, int32_t* __restrict__ matches,
                                                   float* __restrict__ scores, int32_t* __restrict__ count) {
    const Asg a = tab[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int wsum[4];
    __shared__ int base_sh;
    if (tid == 0) base_sh = 0;
    __syncthreads();
    int32_t* mo = matches + (size_t)a.pair * kmax * 2;
    float* so = scores + (size_t)a.pair * kmax;
    for (int c0 = 0; c0 < a.m; c0 += 256) {
        const int i = c0 + tid;
        bool ok = false;
        float sc = 0.f;
        int j = 0;
        if (i < a.m) {
            j = arg[a.ra + i];
            const bool mutual = arg[a.rb + j] == i;
            sc = mutual ? expf(val[a.ra + i]) : 0.f;
            ok = mutual && sc > th;
        }
        int v = ok;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(v, o, 64);
            if (lane >= o) v += t;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int off = base_sh;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (ok) {
            const int slot = off + v - 1;
            mo[2 * slot] = ind[a.ra + i];
            mo[2 * slot + 1] = ind[a.rb + j];
            so[slot] = sc;
        }
        __syncthreads();
        if (tid == 0) base_sh += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) count[a.pair] = base_sh;
}


// ---------------------------------------------------------- pair orientation
// Ordered pair p takes the matches of unordered-pair row rows[p]; with swap[p] the
// image roles are exchanged: (i0, i1) -> (i1, i0), re-sorted ascending in the new image0
// index, which is the order LightGlue itself returns for the swapped call (its matches
// are mutual nearest neighbours, so each index appears at most once: a scatter into
// kmax slots plus an ordered compaction sorts them exactly).  Scores follow their match.
__global__ __launch_bounds__(256) void k_lg_orient(const int32_t* __restrict__ m_in, const float* __restrict__ s_in,
                                                   const int32_t* __restrict__ n_in, const int32_t* __restrict__ rows,
                                                   const uint8_t* __restrict__ swap, int kmax,
                                                   int32_t* __restrict__ m_out, float* __restrict__ s_out,
                                                   int32_t* __restrict__ n_out) {
    __shared__ int slot[2048];
    __shared__ int wsum[256];
    const int p = blockIdx.x, tid = threadIdx.x, r = rows[p];
    const int n = n_in[r];
    const int32_t* mi = m_in + (size_t)r * kmax * 2;
    const float* si = s_in + (size_t)r * kmax;
    int32_t* mo = m_out + (size_t)p * kmax * 2;
    float* so = s_out + (size_t)p * kmax;
    if (!swap[p]) {
        for (int i = tid; i < n; i += 256) {
            mo[2 * i] = mi[2 * i];
            mo[2 * i + 1] = mi[2 * i + 1];
            so[i] = si[i];
        }
        if (tid == 0) n_out[p] = n;
        return;
    }
    for (int i = tid; i < kmax; i += 256) slot[i] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += 256) slot[mi[2 * i + 1]] = i;  // image1 index -> match
    __syncthreads();
    const int per = (kmax + 255) / 256, b0 = tid * per;  // ordered compaction of the slots
    int c = 0;
    for (int j = b0; j < min(b0 + per, kmax); ++j) c += slot[j] >= 0;
    wsum[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < 256; ++t) { const int v = wsum[t]; wsum[t] = acc; acc += v; }
    }
    __syncthreads();
    int o = wsum[tid];
    for (int j = b0; j < min(b0 + per, kmax); ++j) {
        const int i = slot[j];
        if (i < 0) continue;
        mo[2 * o] = j;
        mo[2 * o + 1] = mi[2 * i];
        so[o] = si[i];
        ++o;
    }
    if (tid == 0) n_out[p] = n;
}

// ------------------------------------------------------------------ debug trace
// mlg_dbg_lg_trace_begin / _end (include/mlgate.h): the calling thread's mlg_lightglue
// calls append, after every stage, one 64-bit hash per 64-row tile of the buffer the
// stage wrote (planes x tiles of tile_bytes), so two runs can be compared stage by stage.
struct LgTrace {
    uint64_t* buf = nullptr;
    size_t cap = 0, used = 0;
    bool overflow = false;
    std::vector<int> tags, counts;
};
thread_local LgTrace* t_trace = nullptr;

// tile t = rows [t * rpt, (t + 1) * rpt) of each plane; row r's first row_bytes bytes
// (a multiple of 4) at base + plane * plane_stride + r * row_stride; rows with
// live[r] == 0 skipped when `live` is given (padding rows hold stale workspace)
__global__ __launch_bounds__(256) void k_dbg_hash(const uint8_t* __restrict__ base, int rpt, int row_bytes,
                                                  size_t row_stride, int planes, size_t plane_stride,
                                                  const uint8_t* __restrict__ live, uint64_t* __restrict__ out) {
    const int wpr = row_bytes / 4, words = rpt * wpr;
    uint64_t h = 0;
    for (int p = 0; p < planes; ++p)
        for (int i = threadIdx.x; i < words; i += 256) {
            const size_t r = (size_t)blockIdx.x * rpt + i / wpr;
            if (live && !live[r]) continue;
            uint64_t w = *reinterpret_cast<const uint32_t*>(base + p * plane_stride + r * row_stride + (i % wpr) * 4);
            w ^= (uint64_t)((size_t)p * words + i + 1) * 0x9E3779B97F4A7C15ull;
            w ^= w >> 33;
            w *= 0xff51afd7ed558ccdull;
            w ^= w >> 33;
            w *= 0xc4ceb9fe1a85ec53ull;
            w ^= w >> 33;
            h += w;
        }
    __shared__ uint64_t sh[256];
    sh[threadIdx.x] = h;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// tag = layer * 100 + stage (layer 99: layer 0's self block on the frame layout)
void trace(int tag, const void* base, int rpt, int row_bytes, size_t row_stride, int planes, size_t plane_stride,
           int ntiles, hipStream_t s, const uint8_t* live = nullptr) {
    LgTrace* t = t_trace;
    if (!t || ntiles <= 0 || row_bytes < 4) return;
    if (t->used + (size_t)ntiles > t->cap) {
        t->overflow = true;
        return;
    }
    hipLaunchKernelGGL(k_dbg_hash, dim3((unsigned)ntiles), dim3(256), 0, s, (const uint8_t*)base, rpt, row_bytes & ~3,
                       row_stride, planes, plane_stride, live, t->buf + t->used);
    t->used += ntiles;
    t->tags.push_back(tag);
    t->counts.push_back(ntiles);
}

struct LgBufs {
    // the token buffers, primary and secondary (layer 0's frame layout; the compaction's target)
    float *X, *X2;
    bf16_t *CAT, *CAT2;
    float4 *EF, *EF2;  // rotary factors, lg_fac4 layout
    int32_t *IND, *IND2;
    bf16_t *Q, *K, *VT, *CTX;
    bf16_t* MDH;  // hi half, then the lo half
    uint8_t *LIVE, *KEEP;
    int *ROWSEG, *STATS, *OUTOFF, *ARG;
    float *LZ, *RMAX, *RLOG, *CMAX, *CLOG, *VAL, *SS;
    Seg* SEGS;
    int4 *TASKS, *MOVES;  // TASKS: self tasks, then cross tasks
    float2* PART;
    Asg* ASG;
    float4* NORM;
    int asg_cap;  // pairs per assignment chunk
};

size_t lg_carve(int P, int kmax, void* base, LgBufs* out) {
    const size_t N = (size_t)2 * P * (((size_t)kmax + 63) & ~(size_t)63);
    const size_t ldS = ((size_t)kmax + 3) & ~(size_t)3;
    WsCarver c(base);
    LgBufs b;
    b.asg_cap = std::min(P, 64);
    b.X = c.take<float>(N * LG_D);
    b.CAT = c.take<bf16_t>(N * 512);
    b.EF = c.take<float4>(N * 16);
    b.IND = c.take<int32_t>(N);
    b.X2 = c.take<float>(N * LG_D);
    b.CAT2 = c.take<bf16_t>(N * 512);
    b.EF2 = c.take<float4>(N * 16);
    b.IND2 = c.take<int32_t>(N);
    b.Q = c.take<bf16_t>(N * LG_D);
    b.K = c.take<bf16_t>(N * LG_D);
    b.VT = c.take<bf16_t>(N * LG_D);
    b.CTX = c.take<bf16_t>(N * LG_D);
    b.LIVE = c.take<uint8_t>(N);
    b.ROWSEG = c.take<int>(N);
    b.LZ = c.take<float>(N);
    b.KEEP = c.take<uint8_t>(N);
    b.STATS = c.take<int>((size_t)2 * P * 2);
    b.SEGS = c.take<Seg>((size_t)2 * P);
    b.TASKS = c.take<int4>((size_t)4 * P);
    b.OUTOFF = c.take<int>((size_t)4 * P);
    b.MOVES = c.take<int4>((size_t)2 * P);
    b.MDH = c.take<bf16_t>(2 * N * LG_D);
    b.RMAX = c.take<float>(N);
    b.RLOG = c.take<float>(N);
    b.CMAX = c.take<float>(N);
    b.CLOG = c.take<float>(N);
    b.ARG = c.take<int>(N);
    b.VAL = c.take<float>(N);
    b.PART = c.take<float2>((size_t)b.asg_cap * 2 * ((kmax + ARM - 1) / ARM) * kmax);
    b.ASG = c.take<Asg>((size_t)P);
    b.NORM = c.take<float4>((size_t)2 * P);
    b.SS = c.take<float>((size_t)b.asg_cap * kmax * ldS);
    if (out) *out = b;
    return c.total();
}

float conf_threshold(int i) {
    const double t = 0.8 + 0.1 * exp(-4.0 * i / LG_L);
    return (float)std::min(1.0, std::max(0.0, t));
}

}  // namespace

size_t mlg_lightglue_ws_bytes(int P, int kmax) {
    if (P <= 0 || kmax <= 0 || kmax > 2048) return 0;
    return lg_carve(P, kmax, nullptr, nullptr);
}

int mlg_lightglue_run(const mlg_lg_weights& w, const float* kpts, const float* desc, const int32_t* counts, int kmax,
                      const int32_t* pa, const int32_t* pb, int P, float depth_conf, float width_conf,
                      float filter_thr, int pruning_min, void* ws, size_t ws_bytes, int32_t* matches, float* mscores,
                      int32_t* nmatch, int32_t* stop_layer, hipStream_t s) {
    if (P <= 0 || kmax <= 0 || kmax > 2048) return MLG_EINVAL;
    LgBufs b;  // X / CAT / EF / IND swap with their secondaries at each compaction
    if (lg_carve(P, kmax, ws, &b) > ws_bytes) return MLG_EINVAL;
    // debug trace (mlg_dbg_lg_trace_begin): per-stage hashes of 64-row tiles
    // live rows only (LIVE is the current layout's mask); byte-per-row buffers as 64-B tiles
    auto tr_rows = [&](int tag, const void* p, size_t row_bytes, int np, size_t stride = 0) {
        if (!t_trace) return;
        if (row_bytes < 4) trace(tag, p, 1, 64, 64, 1, 0, np / 64, s);
        else trace(tag, p, 64, (int)row_bytes, stride ? stride : row_bytes, 1, 0, np / 64, s, b.LIVE);
    };
    auto tr_heads = [&](int tag, const void* p, int np) {  // Q / K / V^T: [4 heads][np rows][64] bf16
        if (t_trace) trace(tag, p, 64, 128, 128, 4, (size_t)np * 128, np / 64, s);
    };
    auto tr_tab = [&](int tag, const void* p, size_t bytes) {
        if (t_trace && bytes >= 4) trace(tag, p, 1, (int)bytes, 0, 1, 0, 1, s);
    };
    int tl = 0;  // layer of the next table upload (trace tags)

    // The plan objects own the host tables (pair_plan.h): they are uploaded with
    // hipMemcpyAsync on `s` and rebuilt only after the stream has been synchronised (the
    // per-layer statistics read-back, and one final synchronisation before returning), so
    // the pageable sources outlive every copy that reads them.  h_asg follows the same rule.
    pair_plan::Segments lay;  // the current layout
    pair_plan::AttnTables att;
    pair_plan::FramePlan fp;
    pair_plan::LayerDecision dec;
    std::vector<Asg> h_asg;
    if (hipMemsetAsync(nmatch, 0, sizeof(int32_t) * P, s) != hipSuccess) return MLG_EHIP;
    if (stop_layer) std::fill(stop_layer, stop_layer + P, 0);
    if (!lay.build(counts, pa, pb, P, kmax)) return MLG_EINVAL;
    if (lay.segs.empty()) return MLG_OK;
    std::vector<Seg>& segs = lay.segs;
    std::vector<int>& pair_of = lay.pair_of;  // pair index per active segment pair
    int& Npad = lay.Npad;
    auto upload_layout = [&]() -> int {
        // segments, live-row mask / row -> segment map, self and cross attention tasks
        att.build(segs);
        if (!mlg_upload(b.SEGS, segs, s) || !mlg_upload(b.TASKS, att.tasks, s) || !mlg_upload(b.OUTOFF, att.out_off, s))
            return MLG_EHIP;
        hipLaunchKernelGGL(k_pair_live<int*>, dim3((Npad + 255) / 256), dim3(256), 0, s, b.SEGS, (int)segs.size(),
                           b.LIVE, b.ROWSEG, Npad);
        MLG_LAUNCH_CHECK();
        tr_tab(tl * 100 + 3, b.SEGS, segs.size() * sizeof(Seg));
        tr_tab(tl * 100 + 4, b.TASKS, att.tasks.size() * sizeof(int4));
        tr_tab(tl * 100 + 5, b.OUTOFF, att.out_off.size() * sizeof(int));
        tr_rows(tl * 100 + 6, b.LIVE, 1, Npad);
        return MLG_OK;
    };
    // One self block on the uploaded layout's first `nt` (self) tasks: q / k / v projection
    // with rotary + head split fused in the GEMM epilogue, ragged attention, then out_proj +
    // FFN + residual fused (lg_ffn.hip).  x / cat / ef: the primary buffers, or the secondary
    // ones holding layer 0's frame layout; np rows; trace tags tag + 10 .. 15.
    auto self_block = [&](const mlg_lg_block& bw, float* x, bf16_t* cat, const float4* ef, const int4* tasks,
                          const int* outoff, int nt, int np, int mq, double tok, double work, int tag) -> int {
        {
            MlgProfScope prof(6, s, 2.0 * tok * 768 * 256);
            MLG_TRY(mlg_lg_proj(true, cat, 512, bw.Wqkv, bw.bqkv, (const float*)ef, b.LIVE, b.Q, b.K, b.VT, np, s));
        }
        tr_heads(tag + 10, b.Q, np);
        tr_heads(tag + 11, b.K, np);
        tr_heads(tag + 12, b.VT, np);
        {
            MlgProfScope prof(5, s, work);
            MLG_TRY(mlg_attention_varlen(b.Q, b.K, b.VT, b.CTX, LG_D, np, LG_H, tasks, outoff, nt, mq, s));
        }
        tr_rows(tag + 13, b.CTX, 512, np);
        {
            // algorithmic FLOPs per live token: 2 (256 x 256 + 512 x 512 + 256 x 512) = 917,504.
            // Its HBM bytes per token (ctx + bf16 x in 512 + 512, f32 x read + written 1024 +
            // 1024, bf16 x copy 512 = 3,584) give 256 FLOP/B, near the ridge (2.5 PF / 8 TB/s =
            // 312): the three GEMM phases, not HBM, bound it, so the slot is
            // priced against the MFMA peak
            MlgProfScope prof(8, s, 917504.0 * tok);
            MLG_TRY(mlg_lg_ffn(b.CTX, x, cat, 512, np, bw, s, nullptr));
        }
        tr_rows(tag + 14, x, LG_D * 4, np);
        tr_rows(tag + 15, cat, 512, np, 1024);
        return MLG_OK;
    };
    // Layer 0's self block reads one image only (its tokens, its positional encoding), so
    // it runs once per distinct frame of the call -- a frame layout in the secondary
    // buffers -- and its output rows are copied into every pair segment of that frame:
    // the same kernels on the same rows, so the same bits as running it per pair.
    fp.build(segs, LG_H);
    const bool self0_done = fp.repeats;
    if (fp.repeats) {
        const int nf = (int)fp.fsegs.size(), NpadF = fp.NpadF;
        if (!mlg_upload(b.SEGS, fp.fsegs, s) || !mlg_upload(b.TASKS, fp.tasks, s) ||
            !mlg_upload(b.OUTOFF, fp.out_off, s) || !mlg_upload(b.MOVES, fp.moves, s))
            return MLG_EHIP;
        hipLaunchKernelGGL(k_pair_live<int*>, dim3((NpadF + 255) / 256), dim3(256), 0, s, b.SEGS, nf, b.LIVE, b.ROWSEG,
                           NpadF);
        hipLaunchKernelGGL(k_lg_kpnorm, dim3((unsigned)nf), dim3(256), 0, s, b.SEGS, kpts, kmax, b.NORM);
        hipLaunchKernelGGL(k_lg_init, dim3((unsigned)((kmax + 63) / 64), (unsigned)nf), dim3(256), 0, s, b.SEGS,
                           (const float4*)b.NORM, kpts, desc, kmax, w.Wr, b.X2, b.CAT2, b.EF2, b.IND2);
        MLG_LAUNCH_CHECK();
        tr_tab(9903, b.SEGS, fp.fsegs.size() * sizeof(Seg));
        tr_tab(9904, b.TASKS, fp.tasks.size() * sizeof(int4));
        tr_rows(9901, b.X2, LG_D * 4, NpadF);
        tr_rows(9902, b.CAT2, 512, NpadF, 1024);
        MLG_TRY(self_block(w.self[0], b.X2, b.CAT2, b.EF2, b.TASKS, b.OUTOFF, nf, NpadF, fp.maxqf, fp.tok, fp.work,
                           9900));
    }
    MLG_TRY(upload_layout());
    hipLaunchKernelGGL(k_lg_kpnorm, dim3((unsigned)segs.size()), dim3(256), 0, s, b.SEGS, kpts, kmax, b.NORM);
    hipLaunchKernelGGL(k_lg_init, dim3((unsigned)((kmax + 63) / 64), (unsigned)segs.size()), dim3(256), 0, s, b.SEGS,
                       (const float4*)b.NORM, kpts, desc, kmax, w.Wr, b.X, b.CAT, b.EF, b.IND,
                       self0_done ? (const int4*)b.MOVES : nullptr, b.X2, b.CAT2);
    MLG_LAUNCH_CHECK();
    tr_rows(1, b.X, LG_D * 4, Npad);
    tr_rows(2, b.CAT, 512, Npad, 1024);

    auto live_tokens = [&]() {
        double t = 0;
        for (const Seg& sg : segs) t += sg.len;
        return t;
    };
    auto attn_work = [&](bool cross) {  // 4 * heads * q * kv * 64 per task (QK^T and PV)
        double work = 0;
        for (size_t k = 0; k < segs.size(); k += 2) {
            const double la = segs[k].len, lb = segs[k + 1].len;
            work += 4.0 * LG_H * 64 * (cross ? 2 * la * lb : la * la + lb * lb);
        }
        return work;
    };
    // assignment + filter of the listed segment pairs (k = index of image a's segment)
    auto assign = [&](int i, const std::vector<size_t>& ks) -> int {
        // mdesc = final_proj(x) for every token, as bf16 hi + lo; the 1/4 per side folds into S / 16
        MLG_TRY(mlg_gemm_bias_split_bf16(b.CAT, 512, w.Wfinal[i], w.bfinal[i], b.MDH, b.MDH + (size_t)Npad * LG_D, Npad,
                                         LG_D, LG_D, s));
        if (t_trace) trace(i * 100 + 40, b.MDH, 64, 32, 32, 32, (size_t)Npad * 32, Npad / 64, s);
        // one table upload for all chunks (the per-layer statistics read-back orders its
        // reuse), so chunks follow each other without a host round trip
        h_asg.clear();
        for (size_t c = 0; c < ks.size(); ++c) {
            const Seg sa = segs[ks[c]], sb = segs[ks[c] + 1];
            Asg a;
            a.m = sa.len;
            a.n = sb.len;
            a.ra = sa.off;
            a.rb = sb.off;
            a.soff = (long)(c % b.asg_cap) * kmax * ((kmax + 3) & ~3);
            a.pair = pair_of[ks[c] / 2];
            a.ld = (sb.len + 3) & ~3;
            a.lo_first = sa.frame > sb.frame;
            a.pad = 0;
            h_asg.push_back(a);
            if (stop_layer) stop_layer[a.pair] = i + 1;
        }
        if (!mlg_upload(b.ASG, h_asg, s)) return MLG_EHIP;
        tr_tab(i * 100 + 41, b.ASG, h_asg.size() * sizeof(Asg));
        for (size_t c0 = 0; c0 < ks.size(); c0 += b.asg_cap) {
            const size_t c1 = std::min(ks.size(), c0 + b.asg_cap);
            int maxm = 0, maxn = 0;
            for (size_t c = c0; c < c1; ++c) {
                maxm = std::max(maxm, h_asg[c].m);
                maxn = std::max(maxn, h_asg[c].n);
            }
            const unsigned na = (unsigned)(c1 - c0);
            const Asg* tab = b.ASG + c0;
            const dim3 stiles((maxn + SBM - 1) / SBM, (maxm + SBM - 1) / SBM, na),
                atiles((maxn + ARN - 1) / ARN, (maxm + ARM - 1) / ARM, na),
                lines((std::max(maxm, maxn) + 255) / 256, na, 2);
            hipLaunchKernelGGL(k_asg_sim, stiles, dim3(256), 0, s, tab, b.MDH, b.MDH + (size_t)Npad * LG_D, Npad, b.SS,
                               b.PART, kmax);
            hipLaunchKernelGGL(k_asg_stats, lines, dim3(256), 0, s, tab, b.PART, kmax, b.RMAX, b.RLOG, b.CMAX, b.CLOG);
            hipLaunchKernelGGL(k_asg_arg, atiles, dim3(256), 0, s, tab, b.SS, b.RMAX, b.RLOG, b.CMAX, b.CLOG, b.LZ,
                               b.PART, kmax);
            hipLaunchKernelGGL(k_asg_argfinal, lines, dim3(256), 0, s, tab, b.PART, kmax, b.ARG, b.VAL);
            hipLaunchKernelGGL(k_lg_filter, dim3(na), dim3(256), 0, s, tab, b.ARG, b.VAL, b.IND, filter_thr, kmax,
                               matches, mscores, nmatch);
            MLG_LAUNCH_CHECK();
        }
        return MLG_OK;
    };

    std::vector<int> stats(segs.size() * 2);
    for (int i = 0; i < LG_L && !segs.empty(); ++i) {
        const int nt = (int)segs.size();
        // self block (layer 0's already ran per frame above when frames repeat)
        if (!(i == 0 && self0_done))
            MLG_TRY(self_block(w.self[i], b.X, b.CAT, b.EF, b.TASKS, b.OUTOFF, nt, Npad, att.maxq, live_tokens(),
                               attn_work(false), i * 100));
        // cross block
        {
            MlgProfScope prof(6, s, 2.0 * live_tokens() * 512 * 256);
            MLG_TRY(mlg_lg_proj(false, b.CAT, 512, w.cross[i].Wqkv, w.cross[i].bqkv, nullptr, b.LIVE, b.Q, nullptr,
                                b.VT, Npad, s));
        }
        tr_heads(i * 100 + 20, b.Q, Npad);
        tr_heads(i * 100 + 21, b.VT, Npad);
        {
            MlgProfScope prof(5, s, attn_work(true));
            MLG_TRY(mlg_attention_varlen(b.Q, b.Q, b.VT, b.CTX, LG_D, Npad, LG_H, b.TASKS + nt, b.OUTOFF + nt, nt,
                                         att.maxq, s));
        }
        tr_rows(i * 100 + 22, b.CTX, 512, Npad);
        // layer i's heads on the updated tokens: matchability log-sigmoid (the assignment's
        // certainty term) and, before the last layer, confidences + early-stop / prune flags
        const bool last = i == LG_L - 1;
        const mlg_lg_conf_i heads{b.ROWSEG, last ? nullptr : w.wconf[i], last ? nullptr : w.bconf[i], w.wmatch[i],
                                  w.bmatch[i], last ? 0.f : (depth_conf > 0.f ? conf_threshold(i) : -INFINITY),
                                  width_conf, b.LZ, b.KEEP};
        // (depth_confidence <= 0: upstream computes no token confidences, so its pruning
        // mask is matchability alone -- a threshold of -inf drops the "low confidence is
        // never pruned" term; the stop bit is unused then)
        {
            MlgProfScope prof(8, s, 917504.0 * live_tokens());  // priced as the self block's tail
            MLG_TRY(mlg_lg_ffn(b.CTX, b.X, b.CAT, 512, Npad, w.cross[i], s, &heads));  // + the heads, fused in the tail
        }
        tr_rows(i * 100 + 23, b.X, LG_D * 4, Npad);
        tr_rows(i * 100 + 24, b.CAT, 512, Npad, 1024);
        tr_rows(i * 100 + 25, b.LZ, 4, Npad);
        if (!last) tr_rows(i * 100 + 26, b.KEEP, 1, Npad);

        if (last) {
            std::vector<size_t> ks;
            for (size_t k = 0; k < segs.size(); k += 2) ks.push_back(k);
            MLG_TRY(assign(i, ks));
            break;
        }
        hipLaunchKernelGGL(k_lg_segstats, dim3((unsigned)segs.size()), dim3(256), 0, s, b.SEGS, b.KEEP, b.STATS);
        MLG_LAUNCH_CHECK();
        tr_tab(i * 100 + 27, b.STATS, segs.size() * 2 * sizeof(int));
        if (hipMemcpyAsync(stats.data(), b.STATS, segs.size() * 2 * sizeof(int), hipMemcpyDeviceToHost, s) !=
                hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return MLG_EHIP;
        // early stop per pair; point pruning per segment; the compacted layout
        dec.decide(segs, pair_of, lay.orig_total, stats.data(), depth_conf, width_conf, pruning_min, i);
        if (!dec.stopped.empty()) MLG_TRY(assign(i, dec.stopped));  // the matchability lz came with the confidences
        if (!dec.changed()) continue;
        // compact: drop stopped pairs, prune segments above the threshold
        if (!dec.moves.empty()) {
            if (!dec.stopped.empty() && hipStreamSynchronize(s) != hipSuccess) return MLG_EHIP;  // h_asg in flight
            if (!mlg_upload(b.MOVES, dec.moves, s)) return MLG_EHIP;
            hipLaunchKernelGGL(k_lg_compact, dim3((unsigned)dec.moves.size()), dim3(256), 0, s, b.MOVES, b.KEEP, b.X,
                               b.EF, b.IND, b.X2, b.CAT2, b.EF2, b.IND2);
            MLG_LAUNCH_CHECK();
            std::swap(b.X, b.X2);
            std::swap(b.CAT, b.CAT2);
            std::swap(b.EF, b.EF2);
            std::swap(b.IND, b.IND2);
        }
        // the old layout's upload completed before the read-back above: its vectors may go
        segs.swap(dec.segs);
        pair_of.swap(dec.pair_of);
        Npad = dec.Npad;
        if (stop_layer)
            for (const auto& pl : dec.stop_layer) stop_layer[pl.first] = pl.second;
        tl = i + 1;
        if (!dec.moves.empty()) tr_tab(tl * 100 + 31, b.MOVES, dec.moves.size() * sizeof(int4));
        if (!segs.empty()) MLG_TRY(upload_layout());
        if (!dec.moves.empty() && !segs.empty()) tr_rows(tl * 100 + 30, b.X, LG_D * 4, Npad);
        stats.assign(segs.size() * 2, 0);
    }
    if (t_trace) {
        trace(9990, nmatch, 1, P * 4, 0, 1, 0, 1, s);
    }
    // the last assignment's table (h_asg) and possibly a final layout upload are pageable
    // copies still queued on s: they must complete before the vectors go out of scope
    if (hipStreamSynchronize(s) != hipSuccess) return MLG_EHIP;
    return MLG_OK;
}

int mlg_lg_orient_matches(const int32_t* matches, const float* scores, const int32_t* num_matches,
                          const int32_t* rows, const uint8_t* swap, int P, int kmax, int32_t* matches_out,
                          float* scores_out, int32_t* num_out, void* stream) {
    if (P <= 0) return MLG_OK;
    if (kmax <= 0 || kmax > 2048 || !matches || !scores || !num_matches || !rows || !swap || !matches_out ||
        !scores_out || !num_out)
        return MLG_EINVAL;
    hipLaunchKernelGGL(k_lg_orient, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, matches, scores,
                       num_matches, rows, swap, kmax, matches_out, scores_out, num_out);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

// ---------------------------------------------------------------- debug trace ABI
extern "C" {
int mlg_dbg_lg_trace_begin(void* dev_buf, size_t bytes) {
    if (!dev_buf || bytes < 8) return MLG_EINVAL;
    delete t_trace;
    t_trace = new LgTrace;
    t_trace->buf = (uint64_t*)dev_buf;
    t_trace->cap = bytes / 8;
    return MLG_OK;
}

int mlg_dbg_lg_trace_end(int32_t* tags, int32_t* counts, int max_entries) {
    LgTrace* t = t_trace;
    if (!t) return MLG_EINVAL;
    t_trace = nullptr;
    const int n = (int)t->tags.size();
    const bool overflow = t->overflow;
    if (tags && counts)
        for (int i = 0; i < n && i < max_entries; ++i) {
            tags[i] = t->tags[i];
            counts[i] = t->counts[i];
        }
    delete t;
    return overflow ? MLG_ENOMEM : n;
}
}  // extern "C"
