// MixVPR's native branch (place_recognition.py:227-239, 308-332): the published
// amaralibey/MixVPR model MixVPRModel(backbone='resnet50', out_dim=4096).
//
//   cv2.resize INTER_LINEAR to 320 x 320 on uint8 -> gray / BGRA / BGR -> RGB -> /255 ->
//   ImageNet normalise                                          (k_mix_preprocess)
//   -> torchvision resnet50 cropped after layer3 -> [B, 1024, 20, 20]   (resnet.hip, S = 320)
//   -> x = flatten(2) [B, 1024, 400]; 4 x  x += Linear2(ReLU(Linear1(LayerNorm400(x))))
//   -> channel_proj (1024 -> 1024 over the channel axis), row_proj (400 -> 4), L2 norm.
//
// The head.  Every mixer block acts along the 400 spatial features of one (image, channel)
// row, so one workgroup carries a tile of 64 rows through all 4 blocks (k_mix_head); the
// residual never leaves the chip.  The two projections are linear and commute: row_proj
// is applied first, in the same kernel, while the row is resident (P[c][r], 4 values per
// row), and channel_proj then acts on [1024] x [4] per image instead of [1024] x [400]
// (k_mix_proj: 8 MFLOP per frame instead of 0.84 GFLOP, f32 on the VALU):
//   out[o][r] = sum_c Wc[o][c] P[c][r] + bc[o] s[r] + br[r],  s[r] = sum_i Wr[r][i].
//
// k_mix_head, one workgroup = 4 waves = 64 rows (64 consecutive channels of one image),
// one workgroup per CU.  As in lg_ffn.hip the GEMMs run transposed, C^T = W . T^T with
// v_mfma_f32_32x32x16_bf16: wave w owns output features [128 w, 128 w + 128) for all 64
// rows, so a lane holds feature n = 128 w + 32 t + 8 g + 4 hh + j (t < 4, g < 4, j < 4) of
// rows col and 32 + col.  The f32 residual lives in exactly that accumulator layout, 128
// VGPRs per lane: Linear2 accumulates straight onto it, LayerNorm statistics are
// lane-local sums + one cross-half shuffle + a 4-wave exchange through LDS (two passes:
// mean, then centred variance, as torch), and the gather from the NHWC stream needs no
// transpose -- for one n the 32 lanes of a half-wave read 32 consecutive channels, one
// whole 128-B line, and the second m-tile reads the line beside it.
//   K = N = 400: K is padded to 26 k-steps of 16 (416) and N to 13 column tiles of 32 (416)
// in the pack (zero rows / columns; the LDS tile's columns 400..415 are written as zeros),
// never in the inner loop.  Waves 0..2 own 4 column tiles, wave 3 owns one (features
// 384..415); its other three accumulators stay zero.
//   Weights: 8 matrices x [26][416][16] bf16 = 2.77 MB, re-read by every tile from L2,
// packed k-step-major (mlgate.lightglue.pack_kstep) so a wave's 32 rows x 32 B of one
// k-step are one contiguous 1 KiB; fragments in a 4-step register ring.  The tile's
// one-touch reads (the feature gather) are non-temporal so they do not evict them.
//   Budget per workgroup: LDS 64 KiB (bf16 operand tile [64][512], row_tile.h) + 32 KiB (LayerNorm affine and biases of the 4 blocks) + 8 KiB (row_proj) + 2
// KiB (statistics) = 106 KiB of 160; VGPRs: 128 residual + 128 Linear1 accumulator + 64
// weight ring + 16 token fragments + addresses, under the 512 a single 4-wave workgroup
// per CU may use (__launch_bounds__(256, 1)).
#include "common.h"
#include "kernels.h"
#include "resize_cv.h"
#include "row_tile.h"

namespace {

constexpr int MIX_S = 320;                   // input side
constexpr int MIX_HW = 400, MIX_C = 1024;    // layer3: 20 x 20 positions, 1024 channels
constexpr int MIX_KS = 26, MIX_NP = 416;     // k-steps of 16 and packed rows per matrix
constexpr int MIX_PP = 512;                  // row length of the per-feature parameter arrays
constexpr int MIX_R = 64, MIX_NW = 4;
constexpr size_t MIX_WELEMS = (size_t)MIX_KS * MIX_NP * 16;

// ----------------------------------------------------------- preprocessing ---
// MixVPR._preprocess -> f32 NHWC [B, 320, 320, 3] (what the stem reads), channel c of the
// output = RGB c = stored channel 2 - c (gray: the one channel)
__global__ __launch_bounds__(256) void k_mix_preprocess(const uint8_t* __restrict__ img, int H, int W, int C,
                                                        long img_stride, float* __restrict__ out, long total) {
    __shared__ float lut[3][256];
    for (int i = threadIdx.x; i < 768; i += 256) lut[i >> 8][i & 255] = imagenet_norm(i >> 8, i & 255);
    __syncthreads();
    const int vend = resize_vec_end(MIX_S * C);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % 3), x = (int)((e / 3) % MIX_S), y = (int)((e / (3 * MIX_S)) % MIX_S);
        const long b = e / (3L * MIX_S * MIX_S);
        const int sc = C == 1 ? 0 : 2 - c;
        out[e] = lut[c][resize_cv_sample(img + (size_t)b * img_stride, H, W, C, MIX_S, y, x, sc, vend)];
    }
}

// ------------------------------------------------------------------- head ---
// acc[t][mt] += W[n0 + 32 t + i][k] * T[32 mt + j][k] for t < NTU over the 26 k-steps; W
// packed [26][416][16], T the LDS tile.  lg_ffn.hip's gemm_phase with a k-step count that
// is no multiple of the ring: 6 ring turns + 2 tail steps.
template <int NTU>
__device__ __forceinline__ void mix_gemm(const bf16_t* __restrict__ W, int n0, const char* lds, f32x16 (&acc)[4][2]) {
    constexpr int RING = 4, MT = 2, last = MIX_KS - 1;
    const int lane = threadIdx.x & 63, col = lane & 31, hh = lane >> 5;
    const size_t step = (size_t)MIX_NP * 16;
    const bf16_t* wrow[NTU];
#pragma unroll
    for (int t = 0; t < NTU; ++t) wrow[t] = W + (size_t)(n0 + 32 * t + col) * 16 + 8 * hh;
    const char* xrow = lds + col * ROWB;
    const int sw = col & 15;
    bf16x8 wf[NTU][RING], xa[MT], xb[MT];
#pragma unroll
    for (int t = 0; t < NTU; ++t)
#pragma unroll
        for (int s = 0; s < RING; ++s) wf[t][s] = ld16(wrow[t] + s * step);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
        xa[mt] = *reinterpret_cast<const bf16x8*>(xrow + 32 * mt * ROWB + ((hh ^ sw) << 4));
#define MIX_STEP(KS, S)                                                                                              \
    {                                                                                                                \
        const int ks = (KS);                                                                                         \
        const int cn = ((2 * min(ks + 1, last) + hh) ^ sw) << 4;                                                     \
        bf16x8(&cur)[MT] = ((S)&1) ? xb : xa;                                                                        \
        bf16x8(&nxt)[MT] = ((S)&1) ? xa : xb;                                                                        \
        _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) nxt[mt] =                                                  \
            *reinterpret_cast<const bf16x8*>(xrow + 32 * mt * ROWB + cn);                                            \
        _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int t = 0; t < NTU; ++t)            \
            acc[t][mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[t][S], cur[mt], acc[t][mt], 0, 0, 0);            \
        _Pragma("unroll") for (int t = 0; t < NTU; ++t) wf[t][S] = ld16(wrow[t] + min(ks + RING, last) * step);     \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
    }
#pragma unroll 1
    for (int kb = 0; kb < MIX_KS / RING; ++kb) {
#pragma unroll
        for (int s = 0; s < RING; ++s) MIX_STEP(RING * kb + s, s)
    }
#pragma unroll
    for (int s = 0; s < MIX_KS % RING; ++s) MIX_STEP((MIX_KS / RING) * RING + s, s)
#undef MIX_STEP
}

// the head's weights as the kernels receive them (by value); mlg_mixvpr_head fills it by
// field name from mlg_mixvpr_weights, whose comments give the layouts
struct MixHeadArgs {
    const bf16_t* mix_w;
    const float *mix_p, *row_w, *chan_w, *chan_b, *row_s, *row_b;
};

__global__ __launch_bounds__(64 * MIX_NW, 1) void k_mix_head(const float* __restrict__ feat, MixHeadArgs w,
                                                             float* __restrict__ P) {
    __shared__ __attribute__((aligned(16))) char lds[MIX_R * ROWB];
    __shared__ float red[2][MIX_NW][MIX_R];
    __shared__ __attribute__((aligned(16))) float prm[4 * 4 * MIX_PP];
    __shared__ __attribute__((aligned(16))) float s_wr[4 * MIX_PP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
    for (int i = tid; i < 4 * 4 * MIX_PP; i += 64 * MIX_NW) prm[i] = w.mix_p[i];
    for (int i = tid; i < 4 * MIX_PP; i += 64 * MIX_NW) s_wr[i] = w.row_w[i];
    // tile -> (image, 64 channels); 1024 / 64 = 16 tiles per image, none straddles two
    const int tile = blockIdx.x, b = tile >> 4, c0 = (tile & 15) * MIX_R;
    const int n0 = 128 * wave;

    // 0. gather the tile's f32 rows from the NHWC stream into the accumulator layout
    //    (features past 400: zero, and they stay zero through every block)
    f32x16 x[4][2];
    {
        const float* fb = feat + (size_t)b * MIX_HW * MIX_C + c0 + col;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + 32 * t + 8 * g + 4 * hh;
                const bool gvalid = n0 + 32 * t + 8 * g < MIX_HW;  // wave-uniform (400 % 8 == 0)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        x[t][mt][4 * g + j] =
                            gvalid ? __builtin_nontemporal_load(fb + (size_t)(n + j) * MIX_C + 32 * mt) : 0.f;
            }
    }

#pragma unroll 1
    for (int blk = 0; blk < 4; ++blk) {
        const float* s_g = prm + blk * 4 * MIX_PP;
        const float* s_b = s_g + MIX_PP;
        const float* s_b1 = s_g + 2 * MIX_PP;
        const float* s_b2 = s_g + 3 * MIX_PP;
        const bf16_t* W1 = w.mix_w + (size_t)(2 * blk) * MIX_WELEMS;
        const bf16_t* W2 = W1 + MIX_WELEMS;

        // 1. LayerNorm(400, eps 1e-5) statistics in f32
        float mean[2], rstd[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) sum += x[t][mt][i];
            sum += __shfl_xor(sum, 32, 64);
            if (hh == 0) red[0][wave][32 * mt + col] = sum;
        }
        __syncthreads();  // also: the parameters are staged; every wave has left the previous block's Linear2
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float sum = 0.f;
#pragma unroll
            for (int v = 0; v < MIX_NW; ++v) sum += red[0][v][32 * mt + col];
            mean[mt] = sum * (1.0f / MIX_HW);
            float q = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (n0 + 32 * t + 8 * g >= MIX_HW) continue;  // wave-uniform
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = x[t][mt][4 * g + j] - mean[mt];
                        q += d * d;
                    }
                }
            q += __shfl_xor(q, 32, 64);
            if (hh == 0) red[1][wave][32 * mt + col] = q;
        }
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float q = 0.f;
#pragma unroll
            for (int v = 0; v < MIX_NW; ++v) q += red[1][v][32 * mt + col];
            rstd[mt] = __builtin_amdgcn_rsqf(q * (1.0f / MIX_HW) + 1e-5f);  // lg_ffn.hip: the bare v_rsq_f32
        }
        // 2. the normalised tile, bf16, into LDS (features past 400 as zeros: K padding)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + 32 * t + 8 * g + 4 * hh;
                const bool gvalid = n0 + 32 * t + 8 * g < MIX_HW;
                const float4 lg = *reinterpret_cast<const float4*>(s_g + n);
                const float4 lb = *reinterpret_cast<const float4*>(s_b + n);
                uint2 pk[2];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const f32x16& a = x[t][mt];
                    const float y0 = gvalid ? (a[4 * g] - mean[mt]) * rstd[mt] * lg.x + lb.x : 0.f;
                    const float y1 = gvalid ? (a[4 * g + 1] - mean[mt]) * rstd[mt] * lg.y + lb.y : 0.f;
                    const float y2 = gvalid ? (a[4 * g + 2] - mean[mt]) * rstd[mt] * lg.z + lb.z : 0.f;
                    const float y3 = gvalid ? (a[4 * g + 3] - mean[mt]) * rstd[mt] * lg.w + lb.w : 0.f;
                    pk[mt] = make_uint2(pack_bf16x2(y0, y1), pack_bf16x2(y2, y3));
                }
                cat_pair_write(lds, n >> 3, pk[0], pk[1]);
            }
        __syncthreads();

        // 3. H = ReLU(T . W1^T + b1) -> bf16 over T (padded rows of W1 and b1 are zero: H's
        //    features past 400 come out as zeros)
        {
            f32x16 acc[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[t][mt][i] = 0.f;
            if (wave < 3) mix_gemm<4>(W1, n0, lds, acc);
            else mix_gemm<1>(W1, n0, lds, acc);
            __syncthreads();  // every wave has read T
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = n0 + 32 * t + 8 * g + 4 * hh;
                    const float4 bb = *reinterpret_cast<const float4*>(s_b1 + n);
                    uint2 pk[2];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const f32x16& a = acc[t][mt];
                        pk[mt] = make_uint2(pack_bf16x2(fmaxf(a[4 * g] + bb.x, 0.f), fmaxf(a[4 * g + 1] + bb.y, 0.f)),
                                            pack_bf16x2(fmaxf(a[4 * g + 2] + bb.z, 0.f), fmaxf(a[4 * g + 3] + bb.w, 0.f)));
                    }
                    cat_pair_write(lds, n >> 3, pk[0], pk[1]);
                }
        }
        __syncthreads();

        // 4. x += H . W2^T + b2: the MFMAs accumulate onto the residual itself
        if (wave < 3) mix_gemm<4>(W2, n0, lds, x);
        else mix_gemm<1>(W2, n0, lds, x);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bb = *reinterpret_cast<const float4*>(s_b2 + n0 + 32 * t + 8 * g + 4 * hh);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    x[t][mt][4 * g] += bb.x;
                    x[t][mt][4 * g + 1] += bb.y;
                    x[t][mt][4 * g + 2] += bb.z;
                    x[t][mt][4 * g + 3] += bb.w;
                }
            }
    }

    // 5. row_proj while the rows are resident: P[c][r] = sum_n Wr[r][n] x[c][n] (f32 VALU)
    float pr[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pr[mt][r] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = n0 + 32 * t + 8 * g + 4 * hh;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 wr = *reinterpret_cast<const float4*>(s_wr + r * MIX_PP + n);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const f32x16& a = x[t][mt];
                    pr[mt][r] += a[4 * g] * wr.x + a[4 * g + 1] * wr.y + a[4 * g + 2] * wr.z + a[4 * g + 3] * wr.w;
                }
            }
        }
    __syncthreads();  // every wave has read the last H: the tile becomes f32 scratch [4 waves][64 rows][4]
    float* scr = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = pr[mt][r] + __shfl_xor(pr[mt][r], 32, 64);
            if (hh == 0) scr[(wave * MIX_R + 32 * mt + col) * 4 + r] = v;
        }
    __syncthreads();
    {
        const int row = tid >> 2, r = tid & 3;
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < MIX_NW; ++u) v += scr[(u * MIX_R + row) * 4 + r];
        P[((size_t)tile * MIX_R + row) * 4 + r] = v;
    }
}

// channel_proj on the row-projected features + F.normalize, one workgroup per image, in
// place: desc[b] holds P [1024][4] on entry and the unit descriptor [4096] (o * 4 + r) on exit
__global__ __launch_bounds__(1024) void k_mix_proj(float* __restrict__ desc, MixHeadArgs w) {
    __shared__ __attribute__((aligned(16))) float sP[4 * MIX_C];
    __shared__ __attribute__((aligned(16))) float sO[4 * MIX_C];
    __shared__ float sred[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* d = desc + (size_t)blockIdx.x * 4 * MIX_C;
    *reinterpret_cast<float4*>(sP + 4 * tid) = *reinterpret_cast<const float4*>(d + 4 * tid);
    __syncthreads();
    for (int o = wave; o < MIX_C; o += 16) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 256 * i + 4 * lane;
            const float4 wv = *reinterpret_cast<const float4*>(w.chan_w + (size_t)o * MIX_C + c);
            const float4 p0 = *reinterpret_cast<const float4*>(sP + 4 * c);
            const float4 p1 = *reinterpret_cast<const float4*>(sP + 4 * c + 4);
            const float4 p2 = *reinterpret_cast<const float4*>(sP + 4 * c + 8);
            const float4 p3 = *reinterpret_cast<const float4*>(sP + 4 * c + 12);
            a0 += wv.x * p0.x + wv.y * p1.x + wv.z * p2.x + wv.w * p3.x;
            a1 += wv.x * p0.y + wv.y * p1.y + wv.z * p2.y + wv.w * p3.y;
            a2 += wv.x * p0.z + wv.y * p1.z + wv.z * p2.z + wv.w * p3.z;
            a3 += wv.x * p0.w + wv.y * p1.w + wv.z * p2.w + wv.w * p3.w;
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        a3 = wave_sum(a3);
        if (lane == 0) {
            const float bc = w.chan_b[o];
            *reinterpret_cast<float4*>(sO + 4 * o) =
                make_float4(a0 + bc * w.row_s[0] + w.row_b[0], a1 + bc * w.row_s[1] + w.row_b[1],
                            a2 + bc * w.row_s[2] + w.row_b[2], a3 + bc * w.row_s[3] + w.row_b[3]);
        }
    }
    __syncthreads();
    const float4 v = *reinterpret_cast<const float4*>(sO + 4 * tid);
    const float ss = wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
    if (lane == 0) sred[wave] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += sred[i];
    const float inv = 1.0f / fmaxf(sqrtf(tot), 1e-12f);  // F.normalize(p=2, eps=1e-12)
    *reinterpret_cast<float4*>(d + 4 * tid) = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
}

}  // namespace

int mlg_mixvpr_preprocess(const uint8_t* frames, int B, int H, int W, int C, long frame_stride, float* out,
                          hipStream_t s) {
    if (!frames || !out || B <= 0 || H < 1 || W < 1 || !(C == 1 || C == 3 || C == 4) ||
        frame_stride < (long)H * W * C)
        return MLG_EINVAL;
    const long total = (long)B * MIX_S * MIX_S * 3;
    const int blocks = (int)std::min<long>((total + 255) / 256, 256L * 16);
    hipLaunchKernelGGL(k_mix_preprocess, dim3(blocks), dim3(256), 0, s, frames, H, W, C, frame_stride, out, total);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

int mlg_mixvpr_head(const mlg_mixvpr_weights& pw, const float* feat, int B, float* desc, hipStream_t s) {
    MixHeadArgs w;
    w.mix_w = pw.mix_w;
    w.mix_p = pw.mix_p;
    w.row_w = pw.row_w;
    w.chan_w = pw.chan_w;
    w.chan_b = pw.chan_b;
    w.row_s = pw.row_s;
    w.row_b = pw.row_b;
    if (!feat || !desc || B <= 0 || B > (1 << 20) || !w.mix_w || !w.mix_p || !w.row_w || !w.chan_w || !w.chan_b ||
        !w.row_s || !w.row_b)
        return MLG_EINVAL;
    // the row-projected features go through desc itself ([B][1024][4] f32 = its size)
    hipLaunchKernelGGL(k_mix_head, dim3((unsigned)B * (MIX_C / MIX_R)), dim3(64 * MIX_NW), 0, s, feat, w, desc);
    MLG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mix_proj, dim3((unsigned)B), dim3(1024), 0, s, desc, w);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
