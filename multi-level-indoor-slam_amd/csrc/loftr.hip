// LoFTR detector-free matching (kornia.feature.LoFTR(pretrained='indoor') as the
// reference's LoFTR.detect_and_match runs it, scripts/semantic_gating/
// geometric_verification.py:458-526; semantics restated in oracle/loftr.py).
//
// Features, once per keyframe (mlg_loftr_features), NHWC throughout:
//   k_lf_stem     cv2 BGR2GRAY (fixed point) / 255 -> conv 7x7/2 (1 -> 128, BN folded) +
//                 ReLU on the VALU (0.96 GFLOP per 640x480 frame); f32 + bf16 copy
//   convs         every other conv of ResNetFPN_8_2 as a bf16 MFMA GEMM, k = tap * C + c:
//                 3x3 and strided 1x1 as implicit GEMMs (mlg_conv_implicit, gemm_bf16.hip:
//                 the persistent 256 x 256 / 256 x 128 LDS-DMA tile gathering each K-tile's
//                 16-B channel chunks straight from the NHWC input, padding taps from a zero
//                 line), 1x1 stride 1 as plain GEMMs; bias (folded BN) + shortcut + ReLU /
//                 LeakyReLU fused in the epilogue; 196-channel stages zero-padded to 256
//   k_lf_up_add   FPN merge: lateral + bilinear x2 upsample (align_corners=True) -> bf16
// Matching, per batch of pairs (mlg_loftr_match):
//   coarse tokens x = feat + PE in a side-major f32 residual stream [2][P][L][256] with
//   its bf16 copy in the first half of the MLP input rows CAT [.., 512]; per layer:
//     q, k, v  one GEMM (self) or two (cross: q from x, k / v from the source side),
//              elu + 1 fused on q, k;
//     k_lf_kv    per (segment, head): KV = sum_s phi(k_s)^T (v_s / L), ksum = sum_s phi(k_s)
//                (fixed summation order; segments longer than 256 tokens as per-chunk
//                partials k_lf_kv_part added in chunk order by k_lf_kv_combine);
//     k_lf_apply per (token, head): msg = (phi(q) KV) / (phi(q) . ksum + 1e-6) * L -> bf16
//                (one wave per segment tile and head: KV, ksum wave-uniform);
//     merge GEMM -> k_lf_ln (norm1) -> bf16 into CAT's second half; MLP GEMMs
//     (512 -> 512 ReLU, 512 -> 256); k_lf_ln_res: x += norm2(.), new bf16 copy;
//   dual softmax: S = f0 . f1^T from split-bf16 operands (gemm_bf16.hip; exact-f32 MFMA
//   when L % 4 != 0), sim = S / 256 / 0.1; k_lf_stats (column max, sum exp per row chunk,
//   row block maxima) + k_lf_colfin (chunks merged in chunk order); k_lf_rowbest (row sum,
//   then row max of conf, first argmax) / k_lf_colmaxpart +
//   k_lf_colmaxfin (column max of conf) with conf recomputed identically in both;
//   k_lf_select: conf > 0.2, 2-cell border, mutual max, compacted in row order;
//   fine: k_lf_windows gathers the 5x5 windows (stride 4, zero padding) of the 1/2 maps
//   as bf16, down_proj / merge_feat as GEMMs (the coarse half of merge_feat applied
//   once per match, added to its 25 tokens), the same layer code over 25-token
//   segments (d 128, 8 heads x 16), k_lf_fine_match: softmax(center . window /
//   sqrt(128)), spatial expectation on the [-1, 1] grid, keypoints.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "model_shapes.h"
#include "pair_plan.h"
#include "ws_carve.h"
#include "../../include/mlgate.h"

namespace {

constexpr int STEM_C = 128;

// ------------------------------------------------------------------ stem ----
// One workgroup = 8 output rows x 16 output columns x 128 channels; thread (c, half)
// computes rows 4 half .. + 4 of channel c.  The gray input tile (21 x 37 px) is staged
// in LDS (broadcast reads), the folded 7x7 weights [49][128] read per tap.
__global__ __launch_bounds__(256) void k_lf_stem(const uint8_t* __restrict__ frames, long frame_stride, int H, int W,
                                                 int C, const float* __restrict__ w, const float* __restrict__ bias,
                                                 float* __restrict__ xf, bf16_t* __restrict__ xb) {
    __shared__ float tile[21][37];
    const int Ho = H / 2, Wo = W / 2;
    const int b = blockIdx.z, oy0 = blockIdx.y * 8, ox0 = blockIdx.x * 16;
    const uint8_t* img = frames + (size_t)b * frame_stride;
    for (int e = threadIdx.x; e < 21 * 37; e += 256) {
        const int ty = e / 37, tx = e % 37;
        const int iy = 2 * oy0 - 3 + ty, ix = 2 * ox0 - 3 + tx;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const uint8_t* p = img + ((size_t)iy * W + ix) * C;
            const int g = C >= 3 ? (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14 : p[0];
            v = (float)g / 255.0f;
        }
        tile[ty][tx] = v;
    }
    __syncthreads();
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    float acc[4][16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[r][x] = 0.f;
    for (int ky = 0; ky < 7; ++ky)
        for (int kx = 0; kx < 7; ++kx) {
            const float wv = w[(ky * 7 + kx) * STEM_C + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[r][x] = fmaf(tile[2 * (4 * half + r) + ky][2 * x + kx], wv, acc[r][x]);
        }
    const float bc = bias[c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int oy = oy0 + 4 * half + r;
        if (oy >= Ho) continue;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int ox = ox0 + x;
            if (ox >= Wo) continue;
            const float y = fmaxf(acc[r][x] + bc, 0.f);
            const size_t o = (((size_t)b * Ho + oy) * Wo + ox) * STEM_C + c;
            xf[o] = y;
            xb[o] = f32_to_bf16(y);
        }
    }
}

// ------------------------------------------------------- gray + resize ------
// The reference's LoFTR input for frames whose H or W is not a multiple of 8:
// cv2.cvtColor(BGR2GRAY) then cv2.resize(gray, (W8, H8)) with INTER_LINEAR
// (geometric_verification.py:486-504): OpenCV's fixed-point generic path with 11-bit
// coefficients -- horizontal sums in int, the vertical pass of its 128-bit vector loop
// ((mulhi(S0 >> 4, b0) + mulhi(S1 >> 4, b1) + 2) >> 2) below byte `vend` of a row and
// the scalar FixedPtCast<22> tail above it (oracle/csrc/oracle.c restates the same).
__device__ __forceinline__ int lf_gray(const uint8_t* p, int C) {
    return C >= 3 ? (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14 : p[0];
}
__device__ __forceinline__ int lf_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

__global__ void k_lf_gray_resize(const uint8_t* __restrict__ frames, long frame_stride, int H, int W, int C, int DH,
                                 int DW, int vend, uint8_t* __restrict__ out, int B) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)B * DH * DW) return;
    const int dx = (int)(e % DW), dy = (int)((e / DW) % DH), b = (int)(e / ((long)DW * DH));
    // x: clamped table (cv2 interpolation tables)
    const double sx_scale = 1.0 / ((double)DW / W);
    float fx = (float)((dx + 0.5) * sx_scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= W - 1) { fx = 0.f; sx = W - 1; }
    const int ax0 = lf_s16(__float2int_rn((1.f - fx) * 2048.f)), ax1 = lf_s16(__float2int_rn(fx * 2048.f));
    // y: unclamped weights, clipped source rows
    const double sy_scale = 1.0 / ((double)DH / H);
    float fy = (float)((dy + 0.5) * sy_scale - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    const int by0 = lf_s16(__float2int_rn((1.f - fy) * 2048.f)), by1 = lf_s16(__float2int_rn(fy * 2048.f));
    const int sy0 = min(max(sy, 0), H - 1), sy1 = min(max(sy + 1, 0), H - 1);
    const int sx1 = sx + 1 < W ? sx + 1 : sx;
    const uint8_t* img = frames + (size_t)b * frame_stride;
    const uint8_t* r0 = img + (size_t)sy0 * W * C;
    const uint8_t* r1 = img + (size_t)sy1 * W * C;
    const int s0 = lf_gray(r0 + (size_t)sx * C, C) * ax0 + lf_gray(r0 + (size_t)sx1 * C, C) * ax1;
    const int s1 = lf_gray(r1 + (size_t)sx * C, C) * ax0 + lf_gray(r1 + (size_t)sx1 * C, C) * ax1;
    int v;
    if (dx < vend) {
        const int a0 = lf_s16(s0 >> 4), a1 = lf_s16(s1 >> 4);
        v = (int)(int16_t)(((a0 * by0) >> 16) + ((a1 * by1) >> 16));
        v = (v + 2) >> 2;
    } else {
        v = (s0 * by0 + s1 * by1 + (1 << 21)) >> 22;
    }
    out[e] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---------------------------------------------------------------- FPN add ---
// out_bf16[b, y, x, c] = lat[b, y, x, c] + bilinear_x2(src)[b, y, x, c]  (align_corners:
// source index = dst * (in - 1) / (out - 1) in f32, as torch's upsample_bilinear2d)
__global__ void k_lf_up_add(const float* __restrict__ lat, const float* __restrict__ src, int B, int h, int w, int C,
                            bf16_t* __restrict__ out) {
    const int Ho = 2 * h, Wo = 2 * w, C4 = C / 4;  // 4 channels (16 B of f32) per thread
    const long total = (long)B * Ho * Wo * C4;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C4) * 4;
    long r = e / C4;
    const int x = (int)(r % Wo), y = (int)((r / Wo) % Ho), b = (int)(r / ((long)Wo * Ho));
    const float sh = Ho > 1 ? (float)(h - 1) / (float)(Ho - 1) : 0.f;
    const float sw = Wo > 1 ? (float)(w - 1) / (float)(Wo - 1) : 0.f;
    const float fy = sh * (float)y, fx = sw * (float)x;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 < h - 1 ? y0 + 1 : y0, x1 = x0 < w - 1 ? x0 + 1 : x0;
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* s0 = src + ((size_t)b * h * w) * C + c;
    const float4 v00 = *reinterpret_cast<const float4*>(s0 + ((size_t)y0 * w + x0) * C);
    const float4 v01 = *reinterpret_cast<const float4*>(s0 + ((size_t)y0 * w + x1) * C);
    const float4 v10 = *reinterpret_cast<const float4*>(s0 + ((size_t)y1 * w + x0) * C);
    const float4 v11 = *reinterpret_cast<const float4*>(s0 + ((size_t)y1 * w + x1) * C);
    const float4 l = *reinterpret_cast<const float4*>(lat + r * C + c);
    const float o0 = lf_up_add1(l.x, v00.x, v01.x, v10.x, v11.x, lx0, lx1, ly0, ly1);
    const float o1 = lf_up_add1(l.y, v00.y, v01.y, v10.y, v11.y, lx0, lx1, ly0, ly1);
    const float o2 = lf_up_add1(l.z, v00.z, v01.z, v10.z, v11.z, lx0, lx1, ly0, ly1);
    const float o3 = lf_up_add1(l.w, v00.w, v01.w, v10.w, v11.w, lx0, lx1, ly0, ly1);
    *reinterpret_cast<uint2*>(out + r * C + c) = make_uint2(pack_bf16x2(o0, o1), pack_bf16x2(o2, o3));
}

// ------------------------------------------------------- tokens + PE --------
// x[row] = feat[frame(row)][t] + pe[t] (f32) and bf16 copy into cat[row][0..255]
__global__ void k_lf_tokens(const float* __restrict__ coarse, const int32_t* __restrict__ frame_of, int L,
                            const float* __restrict__ pe, float* __restrict__ x, bf16_t* __restrict__ cat, int rows) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (row, 4 channels)
    if (e >= (long)rows * 64) return;
    const int row = (int)(e / 64), c4 = (int)(e % 64), seg = row / L, t = row - seg * L;
    const float4 f = reinterpret_cast<const float4*>(coarse + ((size_t)frame_of[seg] * L + t) * 256)[c4];
    const float4 p = reinterpret_cast<const float4*>(pe + (size_t)t * 256)[c4];
    const float4 y = make_float4(f.x + p.x, f.y + p.y, f.z + p.z, f.w + p.w);
    reinterpret_cast<float4*>(x + (size_t)row * 256)[c4] = y;
    reinterpret_cast<uint2*>(cat + (size_t)row * 512)[c4] = make_uint2(pack_bf16x2(y.x, y.y), pack_bf16x2(y.z, y.w));
}

// Layer 0 of the coarse transformer is a self layer: its output rows depend on the frame
// alone.  k_lf_stash copies the distinct frames' rows (f32 x and its bf16 copy, the first
// half of cat) aside; k_lf_gather_rows lays them out per pair side (segment g <- frame row
// block umap[g]) for layers 1..
__global__ void k_lf_stash(const float* __restrict__ x, const bf16_t* __restrict__ cat, long rows,
                           float* __restrict__ tx, bf16_t* __restrict__ tc) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (row, 16 B of x) then (row, 16 B of cat)
    if (e < rows * 64) {
        reinterpret_cast<float4*>(tx)[e] = reinterpret_cast<const float4*>(x)[e];
    } else if (e < rows * 96) {
        const long f = e - rows * 64, r = f >> 5;
        const int c = (int)(f & 31);
        reinterpret_cast<uint4*>(tc + r * 256)[c] = reinterpret_cast<const uint4*>(cat + r * 512)[c];
    }
}

__global__ void k_lf_gather_rows(const float* __restrict__ tx, const bf16_t* __restrict__ tc,
                                 const int32_t* __restrict__ umap, int L, long rows, float* __restrict__ x,
                                 bf16_t* __restrict__ cat) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < rows * 64) {
        const long r = e >> 6;
        const int c = (int)(e & 63), g = (int)(r / L), t = (int)(r - (long)g * L);
        reinterpret_cast<float4*>(x + r * 256)[c] =
            reinterpret_cast<const float4*>(tx + ((long)umap[g] * L + t) * 256)[c];
    } else if (e < rows * 96) {
        const long f = e - rows * 64, r = f >> 5;
        const int c = (int)(f & 31), g = (int)(r / L), t = (int)(r - (long)g * L);
        reinterpret_cast<uint4*>(cat + r * 512)[c] = reinterpret_cast<const uint4*>(tc + ((long)umap[g] * L + t) * 256)[c];
    }
}

// ------------------------------------------------------ linear attention ----
// per (segment, head): KV[dk][dv] = sum_s phik[s][dk] * (v[s][dv] / L) (v arrives divided by
// L from the qkv GEMM epilogue), ksum[dk] = sum_s phik[s][dk]; phik / v rows of segment g start at (g * L + s) * ld + col offset.  Thread
// (dk, dv-quad) of a 256-thread group; tokens staged 64 at a time through LDS.
template <int DH>
__global__ __launch_bounds__(256) void k_lf_kv(const float* __restrict__ k, const float* __restrict__ v, int ldk,
                                               int ldv, int L, int heads, const int32_t* __restrict__ kseg,
                                               float* __restrict__ KV, float* __restrict__ ksum) {
    __shared__ float sk[64][DH + 1], sv[64][DH + 1];
    const int g = blockIdx.x / heads, h = blockIdx.x % heads;
    const int src = kseg ? kseg[g] : g;
    constexpr int NQ = DH * DH / 4;  // (dk, quad) items
    const int tid = threadIdx.x;
    float acc[(NQ + 255) / 256][4] = {};
    float ks = 0.f;
    const float invL = 1.0f / (float)L;
    for (int s0 = 0; s0 < L; s0 += 64) {
        const int n = min(64, L - s0);
        __syncthreads();
        for (int e = tid; e < 64 * DH; e += 256) {
            const int s = e / DH, d = e % DH;
            float a = 0.f, b = 0.f;
            if (s < n) {
                const size_t row = (size_t)src * L + s0 + s;
                a = k[row * ldk + h * DH + d];
                b = v[row * ldv + h * DH + d];  // already v / L (qkv GEMM epilogue)
            }
            sk[s][d] = a;
            sv[s][d] = b;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < (NQ + 255) / 256; ++it) {
            const int q = tid + 256 * it;
            if (q >= NQ) break;
            const int dk = q / (DH / 4), dv = (q % (DH / 4)) * 4;
            for (int s = 0; s < n; ++s) {
                const float a = sk[s][dk];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[it][j] = fmaf(a, sv[s][dv + j], acc[it][j]);
            }
        }
        if (tid < DH)
            for (int s = 0; s < n; ++s) ks += sk[s][tid];
    }
    (void)invL;
#pragma unroll
    for (int it = 0; it < (NQ + 255) / 256; ++it) {
        const int q = tid + 256 * it;
        if (q >= NQ) break;
        const int dk = q / (DH / 4), dv = (q % (DH / 4)) * 4;
        float* o = KV + (((size_t)g * heads + h) * DH + dk) * DH + dv;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = acc[it][j];
    }
    if (tid < DH) ksum[((size_t)g * heads + h) * DH + tid] = ks;
}

// Chunked form of k_lf_kv for long segments: one wave per (segment, head, chunk of
// LF_KV_CHUNK tokens); lane (bk, bv) owns the B x B block (B = DH / 8) KV[bk B .., bv B ..]
// and reads its k / v quads straight from the rows (the 8 lanes sharing bk read the same
// bytes); ksum by the lanes with bv == 0.  Partial sums [seg, head, chunk][DH * DH + DH]
// (tokens in order inside a chunk); k_lf_kv_combine adds the chunks in chunk order.
constexpr int LF_KV_CHUNK = 256;
// The 8 tokens' k / v head slices of a step come in as whole 1-KiB wave
// loads (lane = 16 B of the 8 x DH k | v block) through a per-wave LDS image, instead of
// one 16-B load per lane per token and operand (8 lanes sharing each address, 128 B per
// wave-instruction); the next step's loads are in flight while this step's FMAs run.
// Same per-lane FMA order, so the same sums (-3 % matching, profiles/r05n_ab_loftr_kv_stage.txt).
template <int DH>
__global__ __launch_bounds__(256) void k_lf_kv_part(const float* __restrict__ k, const float* __restrict__ v, int ldk,
                                                    int ldv, int L, int heads, int nseg, int nch,
                                                    float* __restrict__ part) {
    constexpr int B = DH / 8;
    constexpr int NI = DH / 16;  // float4 per lane per 8-token step (k and v together: 16 DH floats)
    __shared__ __attribute__((aligned(16))) float stage[4][2 * 8 * DH];
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= nseg * heads * nch) return;
    const int c = w % nch, gh = w / nch, h = gh % heads, g = gh / heads;
    const int bk = lane >> 3, bv = lane & 7;
    const int s0 = c * LF_KV_CHUNK, s1 = min(L, s0 + LF_KV_CHUNK);
    float acc[B][B] = {};
    float ks[B] = {};
    int s = s0;
    float* st = stage[threadIdx.x >> 6];
    // lane's float4 i of a step: flat f = 4 (lane + 64 i) of [k | v][8 tokens][DH]
    auto fetch = [&](int s_, float4 (&r)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int f = 4 * (lane + 64 * i), kv = f / (8 * DH), u = (f % (8 * DH)) / DH, d = f % DH;
            const size_t row = (size_t)g * L + s_ + u;
            r[i] = *reinterpret_cast<const float4*>((kv ? v + row * ldv : k + row * ldk) + h * DH + d);
        }
    };
    float4 nxt[NI];
    if (s + 8 <= s1) fetch(s, nxt);
    for (; s + 8 <= s1; s += 8) {
#pragma unroll
        for (int i = 0; i < NI; ++i) *reinterpret_cast<float4*>(st + 4 * (lane + 64 * i)) = nxt[i];
        __builtin_amdgcn_wave_barrier();
        if (s + 16 <= s1) fetch(s + 8, nxt);
        float a[8][B], b[8][B];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int i = 0; i < B; ++i) {
                a[u][i] = st[u * DH + bk * B + i];
                b[u][i] = st[8 * DH + u * DH + bv * B + i];
            }
        __builtin_amdgcn_wave_barrier();  // reads issued before the next step's writes
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int i = 0; i < B; ++i) {
                ks[i] += a[u][i];
#pragma unroll
                for (int j = 0; j < B; ++j) acc[i][j] = fmaf(a[u][i], b[u][j], acc[i][j]);
            }
    }
    for (; s < s1; ++s) {
        const size_t row = (size_t)g * L + s;
        const float* kr = k + row * ldk + h * DH + bk * B;
        const float* vr = v + row * ldv + h * DH + bv * B;
        float a[B], b[B];
#pragma unroll
        for (int i = 0; i < B; ++i) {
            a[i] = kr[i];
            b[i] = vr[i];
        }
#pragma unroll
        for (int i = 0; i < B; ++i) {
            ks[i] += a[i];
#pragma unroll
            for (int j = 0; j < B; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
    }
    float* o = part + (size_t)w * (DH * DH + DH);
#pragma unroll
    for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) o[(bk * B + i) * DH + bv * B + j] = acc[i][j];
    if (bv == 0)
#pragma unroll
        for (int i = 0; i < B; ++i) o[DH * DH + bk * B + i] = ks[i];
}

template <int DH>
__global__ __launch_bounds__(256) void k_lf_kv_combine(const float* __restrict__ part, int nsh, int nch,
                                                       float* __restrict__ KV, float* __restrict__ ksum) {
    constexpr int E = DH * DH + DH;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)nsh * E) return;
    const long gh = e / E;
    const int i = (int)(e % E);
    const float* p = part + gh * nch * E + i;
    float s = p[0];
    for (int c = 1; c < nch; ++c) s += p[(size_t)c * E];
    if (i < DH * DH)
        KV[gh * DH * DH + i] = s;
    else
        ksum[gh * DH + (i - DH * DH)] = s;
}

// msg[row][h * DH + dv] = (sum_dk phiq[dk] KV[dk][dv]) * (1 / (phiq . ksum + 1e-6)) * L.
// One wave per (segment, 64-token tile, head), lane = token: the segment's KV and ksum
// are wave-uniform (scalar loads, SGPR operands of the FMAs); sums over dk in order.
template <int DH>
__global__ __launch_bounds__(256) void k_lf_apply(const float* __restrict__ q, int ldq, const float* __restrict__ KV,
                                                  const float* __restrict__ ksum, int L, int heads, int nseg,
                                                  bf16_t* __restrict__ msg) {
    const int tiles = (L + 63) / 64;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= nseg * tiles * heads) return;
    const int h = w % heads, gt = w / heads, t = gt % tiles, g = gt / tiles;
    const int s = t * 64 + (threadIdx.x & 63);
    if (s >= L) return;
    const size_t row = (size_t)g * L + s;
    const float* qr = q + row * ldq + h * DH;
    const float* kv = KV + ((size_t)g * heads + h) * DH * DH;
    const float* ks = ksum + ((size_t)g * heads + h) * DH;
    float qv[DH];
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        const float4 x = *reinterpret_cast<const float4*>(qr + d);
        qv[d] = x.x;
        qv[d + 1] = x.y;
        qv[d + 2] = x.z;
        qv[d + 3] = x.w;
    }
    float z = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) z = fmaf(qv[d], ks[d], z);
    const float zi = 1.0f / (z + 1e-6f);
    bf16_t* o = msg + row * (heads * DH) + h * DH;
#pragma unroll
    for (int dv0 = 0; dv0 < DH; dv0 += 8) {
        float a[8] = {};
#pragma unroll
        for (int d = 0; d < DH; ++d)
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = fmaf(qv[d], kv[d * DH + dv0 + j], a[j]);
        uint4 pk;
        pk.x = pack_bf16x2(a[0] * zi * (float)L, a[1] * zi * (float)L);
        pk.y = pack_bf16x2(a[2] * zi * (float)L, a[3] * zi * (float)L);
        pk.z = pack_bf16x2(a[4] * zi * (float)L, a[5] * zi * (float)L);
        pk.w = pack_bf16x2(a[6] * zi * (float)L, a[7] * zi * (float)L);
        *reinterpret_cast<uint4*>(o + dv0) = pk;
    }
}

// ------------------------------------------------------------- LayerNorm ----
// one wave per row of D (128 or 256) f32: torch's two-pass mean / variance (biased), eps
// 1e-5.  mode 0: y -> bf16 out[row * ldo + col0 ..]; mode 1: x[row] += y, bf16(x) ->
// out[row * ldo ..] (the residual update and the next layer's bf16 operand).
template <int D>
__global__ __launch_bounds__(256) void k_lf_ln(const float* __restrict__ in, const float* __restrict__ g,
                                               const float* __restrict__ b, long rows, int mode, float* __restrict__ x,
                                               bf16_t* __restrict__ out, int ldo) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    constexpr int PER = D / 64;
    float v[PER];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        v[i] = in[row * D + lane * PER + i];
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const float d = v[i] - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane * PER + i;
        float y = (v[i] - mean) * rstd * g[c] + b[c];
        if (mode == 1) {
            y = x[row * D + c] + y;
            x[row * D + c] = y;
        }
        out[row * ldo + c] = f32_to_bf16(y);
    }
}

// f32 [rows][256] -> bf16 [rows][512] = [hi | lo] (x = hi + lo to 2^-17; the LoFTR
// coarse similarity's split operands)
__global__ __launch_bounds__(256) void k_lf_split_rows(const float* __restrict__ x, long rows,
                                                       bf16_t* __restrict__ out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // one float4 per thread
    if (e >= rows * 64) return;
    const long r = e >> 6;
    const int c = (int)(e & 63) * 4;
    const float4 v = *reinterpret_cast<const float4*>(x + r * 256 + c);
    uint2 hi, lo;
    split_bf16x4(v.x, v.y, v.z, v.w, hi, lo);
    *reinterpret_cast<uint2*>(out + r * 512 + c) = hi;
    *reinterpret_cast<uint2*>(out + r * 512 + 256 + c) = lo;
}

// ------------------------------------------------------- dual softmax -------
// S holds the similarity x = (f0 . f1 / 256) / 0.1 (mlg_similarity_f32_loftr: the
// reference divides each side by 16 and the product by the temperature); per row i:
// max_j x, sum_j exp(x - max); per column likewise; conf = softmax over dim 1 (column-
// wise) * softmax over dim 2 (row-wise), as torch.  Softmax sums are two-pass (max, then
// sum of exp(x - max)), with the row / column held in registers (one HBM read each).
// Row-best / column-best of conf: conf_ij is proportional to exp(2 x_ij - rkey_i - ckey_j)
// with rkey = rmax + log rsum, ckey = cmax + log csum, so a pass keeps the best key and
// evaluates the exact conf only where the key is within LF_KEY_BAND of it (f32 conf
// rounding moves the key by ~1e-6): the same argmax / max as the exact conf everywhere,
// two exponentials per candidate instead of per cell.
constexpr int LF_ROWREG = 24;        // float4 per lane: rows of up to 6144 cells in registers
constexpr float LF_KEY_BAND = 1e-3f;  // + 1e-5 |key|
constexpr int LF_RCH = 64;           // rows per column chunk
// Pairs per dual-softmax group: the similarity of up to MLG_LF_PGRP pairs is resident at
// once ([G][L][L] f32, 92 MB per pair at 480 x 640) and every statistics / selection kernel
// takes the group in blockIdx.z (pair z: S + z L^2, per-row / per-column arrays + z L, chunk
// partials + z nch L), so the small per-pair kernels fill the chip and the launch
// boundaries amortise over the group; per-pair arithmetic unchanged (same bits).
constexpr int MLG_LF_PGRP = 8;
#define LF_Z ((size_t)blockIdx.z)

__device__ __forceinline__ float lf_band(float k) { return LF_KEY_BAND + 1e-5f * fabsf(k); }

// The softmax SUMS' exponentials (row / column sum of exp(x - max), the chunk merge): the
// hardware exp2 of x log2 e (__expf: v_mul + v_exp_f32, relative error ~|x| 2^-24 per term)
// instead of the libm-accurate expf (~10 VALU), as these sums made the statistics passes
// VALU-bound (k_lf_rowbest -10 %, matches identical, profiles/r06n_ab_loftr_fast_sum_exp.txt);
// the exact conf of a candidate keeps expf.
__device__ __forceinline__ float lf_sexp(float x) { return __expf(x); }

// conf as the reference computes it: softmax(sim, 1) * softmax(sim, 2)
__device__ __forceinline__ float lf_conf(float x, float rm, float rz, float cm, float cz) {
    return (expf(x - cm) / cz) * (expf(x - rm) / rz);
}

// Column statistics in two steps so that the whole chip reads S: grid (column blocks of
// 256, row chunks of LF_RCH); thread = column, coalesced 1 KiB row reads, the chunk's 64
// values in registers.  Chunk c's (max, sum exp(x - max)) -> pm / pz [c][L]; k_lf_colfin
// merges the chunks (max, then sum_c pz_c exp(pm_c - max)).
// The row maxima come from the same tile, so that one read of S yields both (the dual
// softmax in three reads of S instead of four: -1.2 %, digest identical, profiles/
// r05g_ab_loftr_dual_softmax_3read.txt): after the column statistics the 64 x 64 (row x lane) values of a wave
// fold in six butterfly steps -- step b exchanges half of the rows with lane ^ b and keeps
// the max -- until lane l holds row l's max over the wave's 64 columns; the four waves
// meet in LDS and prm[column block][row] gets the block's max.  Max is exact in any order,
// so rmax = max over blocks equals a whole-row pass's bit for bit.
__global__ __launch_bounds__(256) void k_lf_stats(const float* __restrict__ S, int L, int lds, float* __restrict__ pm,
                                                  float* __restrict__ pz, float* __restrict__ prm) {
    __shared__ float red[4][LF_RCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const int r0 = c * LF_RCH, n = min(L - r0, LF_RCH);
    const bool ok = col < L;
    S += LF_Z * L * lds;
    pm += LF_Z * gridDim.y * L;
    pz += LF_Z * gridDim.y * L;
    prm += LF_Z * gridDim.x * L;
    float v[LF_RCH], m = -INFINITY, z = 0.f;
#pragma unroll
    for (int i = 0; i < LF_RCH; ++i) {
        v[i] = (ok && i < n) ? S[(size_t)(r0 + i) * lds + col] : -INFINITY;
        m = fmaxf(m, v[i]);
    }
#pragma unroll
    for (int i = 0; i < LF_RCH; ++i)
        if (i < n) z += lf_sexp(v[i] - m);
    if (ok) {
        pm[(size_t)c * L + col] = m;
        pz[(size_t)c * L + col] = z;
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const bool up = (lane & h) != 0;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const float keep = up ? v[h + i] : v[i], send = up ? v[i] : v[h + i];
            v[i] = fmaxf(keep, __shfl_xor(send, h, 64));
        }
    }
    red[wave][lane] = v[0];
    __syncthreads();
    if (wave == 0 && lane < n)
        prm[(size_t)blockIdx.x * L + r0 + lane] =
            fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
}

// 64 columns x 4 chunk groups per workgroup (group g: chunks g, g + 4, ..): the chunk
// loads of a column run in parallel; the four partials combine in group order
__global__ __launch_bounds__(256) void k_lf_colfin(const float* __restrict__ pm, const float* __restrict__ pz, int L,
                                                   int lds, int nch, float* __restrict__ cmax, float* __restrict__ csum,
                                                   float* __restrict__ ckey) {
    __shared__ float part[4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, col = blockIdx.x * 64 + cl;
    const bool ok = col < L;
    pm += LF_Z * nch * L;
    pz += LF_Z * nch * L;
    cmax += LF_Z * L;
    csum += LF_Z * L;
    ckey += LF_Z * lds;  // rows of lds: k_lf_rowbest reads it as float4 over [0, lds)
    float m = -INFINITY;
    if (ok)
#pragma unroll 4
        for (int c = g; c < nch; c += 4) m = fmaxf(m, pm[(size_t)c * L + col]);
    part[g][cl] = m;
    __syncthreads();
    m = fmaxf(fmaxf(part[0][cl], part[1][cl]), fmaxf(part[2][cl], part[3][cl]));
    __syncthreads();
    float z = 0.f;
    if (ok)
#pragma unroll 4
        for (int c = g; c < nch; c += 4) z += pz[(size_t)c * L + col] * lf_sexp(pm[(size_t)c * L + col] - m);
    part[g][cl] = z;
    __syncthreads();
    if (g == 0 && ok) {
        z = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
        cmax[col] = m;
        csum[col] = z;
        ckey[col] = m + logf(z);
    }
}

// One wave per row; the row lives in v[] (lane l: float4 l + 64 k); rows longer than 256
// LF_ROWREG cells take the loops over memory.  The row max comes from k_lf_stats' block
// maxima prm[ncb][L] and the row sum is formed here from the registers that hold the row
// anyway; rmax / rsum / rkey are written for k_lf_colmaxpart.
__global__ __launch_bounds__(256) void k_lf_rowbest(const float* __restrict__ S, int L, int lds, float* __restrict__ rmax,
                                                    float* __restrict__ rsum, float* __restrict__ rkey,
                                                    const float* __restrict__ prm, int ncb,
                                                    const float* __restrict__ cmax, const float* __restrict__ csum,
                                                    const float* __restrict__ ckey, float* __restrict__ bval,
                                                    int32_t* __restrict__ bidx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= L) return;
    S += LF_Z * L * lds;
    rmax += LF_Z * L;
    rsum += LF_Z * L;
    rkey += LF_Z * L;
    prm += LF_Z * ncb * L;
    cmax += LF_Z * L;
    csum += LF_Z * L;
    ckey += LF_Z * lds;
    bval += LF_Z * L;
    bidx += LF_Z * L;
    const float* s = S + (size_t)row * lds;
    float rm, rz;
    // register rows: 16-B reads over [0, lds); the pad columns [L, lds) hold -inf, so they
    // add nothing to the max / sum and never pass the key band (2 (-inf) - key = -inf or NaN)
    const bool reg = (lds & 3) == 0 && lds <= 256 * LF_ROWREG;
    float4 v[LF_ROWREG];
    if (reg) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
#pragma unroll
        for (int k = 0; k < LF_ROWREG; ++k)
            if (lane + 64 * k < lds / 4) v[k] = s4[lane + 64 * k];
    }
    {
        float m = -INFINITY;
        for (int b = lane; b < ncb; b += 64) m = fmaxf(m, prm[(size_t)b * L + row]);
        m = wave_max(m);
        float z = 0.f;
        if (reg) {
#pragma unroll
            for (int k = 0; k < LF_ROWREG; ++k)
                if (lane + 64 * k < lds / 4)
                    z += lf_sexp(v[k].x - m) + lf_sexp(v[k].y - m) + lf_sexp(v[k].z - m) + lf_sexp(v[k].w - m);
        } else {
            for (int j = lane; j < L; j += 64) z += lf_sexp(s[j] - m);
        }
        z = wave_sum(z);
        rm = m;
        rz = z;
        if (lane == 0) {
            rmax[row] = m;
            rsum[row] = z;
            rkey[row] = m + logf(z);
        }
    }
    float bv = -1.f;
    int bi = 0x7fffffff;
    auto take = [&](float x, int j) {
        const float c = lf_conf(x, rm, rz, cmax[j], csum[j]);
        if (c > bv || (c == bv && j < bi)) { bv = c; bi = j; }
    };
    float kb = -INFINITY;
    if (reg) {
        const float4* k4 = reinterpret_cast<const float4*>(ckey);
#pragma unroll
        for (int k = 0; k < LF_ROWREG; ++k) {
            const int j = lane + 64 * k;
            if (j < lds / 4) {
                const float4 ck = k4[j];
                kb = fmaxf(kb, fmaxf(fmaxf(2.f * v[k].x - ck.x, 2.f * v[k].y - ck.y),
                                     fmaxf(2.f * v[k].z - ck.z, 2.f * v[k].w - ck.w)));
            }
        }
        kb = wave_max(kb);
        const float lim = kb - lf_band(kb);
#pragma unroll
        for (int k = 0; k < LF_ROWREG; ++k) {
            const int j = lane + 64 * k;
            if (j < lds / 4) {
                const float4 ck = k4[j];
                if (2.f * v[k].x - ck.x >= lim) take(v[k].x, 4 * j);
                if (2.f * v[k].y - ck.y >= lim) take(v[k].y, 4 * j + 1);
                if (2.f * v[k].z - ck.z >= lim) take(v[k].z, 4 * j + 2);
                if (2.f * v[k].w - ck.w >= lim) take(v[k].w, 4 * j + 3);
            }
        }
    } else {
        for (int j = lane; j < L; j += 64) kb = fmaxf(kb, 2.f * s[j] - ckey[j]);
        kb = wave_max(kb);
        const float lim = kb - lf_band(kb);
        for (int j = lane; j < L; j += 64)
            if (2.f * s[j] - ckey[j] >= lim) take(s[j], j);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // max value, first index on ties
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        bval[row] = bv;
        bidx[row] = bi;
    }
}

// column max of conf per row chunk (max is exact in any order)
__global__ __launch_bounds__(256) void k_lf_colmaxpart(const float* __restrict__ S, int L, int lds,
                                                       const float* __restrict__ rmax, const float* __restrict__ rsum,
                                                       const float* __restrict__ rkey, const float* __restrict__ cmax,
                                                       const float* __restrict__ csum, float* __restrict__ pb) {
    __shared__ float rk[LF_RCH];
    const int col = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const int r0 = c * LF_RCH, n = min(L - r0, LF_RCH);
    S += LF_Z * L * lds;
    rmax += LF_Z * L;
    rsum += LF_Z * L;
    rkey += LF_Z * L;
    cmax += LF_Z * L;
    csum += LF_Z * L;
    pb += LF_Z * gridDim.y * L;
    if (threadIdx.x < LF_RCH) rk[threadIdx.x] = threadIdx.x < n ? rkey[r0 + threadIdx.x] : INFINITY;
    __syncthreads();
    if (col >= L) return;
    const float cm = cmax[col], cz = csum[col];
    float v[LF_RCH], kb = -INFINITY;
#pragma unroll
    for (int i = 0; i < LF_RCH; ++i) {
        v[i] = i < n ? S[(size_t)(r0 + i) * lds + col] : 0.f;
        kb = fmaxf(kb, 2.f * v[i] - rk[i]);
    }
    const float lim = kb - lf_band(kb);
    float m = -1.f;
#pragma unroll
    for (int i = 0; i < LF_RCH; ++i)
        if (i < n && 2.f * v[i] - rk[i] >= lim) m = fmaxf(m, lf_conf(v[i], rmax[r0 + i], rsum[r0 + i], cm, cz));
    pb[(size_t)c * L + col] = m;
}

__global__ __launch_bounds__(256) void k_lf_colmaxfin(const float* __restrict__ pb, int L, int nch,
                                                      float* __restrict__ cbest) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= L) return;
    pb += LF_Z * nch * L;
    cbest += LF_Z * L;
    float m = -1.f;
#pragma unroll 8
    for (int c = 0; c < nch; ++c) m = fmaxf(m, pb[(size_t)c * L + col]);
    cbest[col] = m;
}

// Mutual-nearest selection with threshold and border, compacted in row order (one
// workgroup per pair): match (i, j = best_i) iff conf > thr, neither cell within
// `border` cells of its map's edge, conf == column max of j.
__global__ __launch_bounds__(1024) void k_lf_select(const float* __restrict__ bval, const int32_t* __restrict__ bidx,
                                                    const float* __restrict__ cbest, int L, int hc, int wc, float thr,
                                                    int border, int32_t* __restrict__ mi, int32_t* __restrict__ mj,
                                                    float* __restrict__ mconf, int32_t* __restrict__ count) {
    __shared__ int warp_tot[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bval += LF_Z * L;
    bidx += LF_Z * L;
    cbest += LF_Z * L;
    mi += LF_Z * L;
    mj += LF_Z * L;
    mconf += LF_Z * L;
    count += LF_Z;
    if (tid == 0) base = 0;
    __syncthreads();
    auto inner = [&](int id) {
        const int r = id / wc, c = id % wc;
        return r >= border && r < hc - border && c >= border && c < wc - border;
    };
    for (int i0 = 0; i0 < L; i0 += 1024) {
        const int i = i0 + tid;
        bool ok = false;
        float v = 0.f;
        int j = 0;
        if (i < L) {
            v = bval[i];
            j = bidx[i];
            ok = v > thr && j >= 0 && j < L && inner(i) && inner(j) && v == cbest[j];
        }
        const unsigned long long bal = __ballot(ok);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) warp_tot[wave] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += warp_tot[w];
        if (ok) {
            mi[off + pre] = i;
            mj[off + pre] = j;
            mconf[off + pre] = v;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += warp_tot[w];
            base += t;
        }
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

// ---------------------------------------------------------------- fine ------
// Match m of a chunk = (pair mp[m], slot ms[m]): cell i = mi[pair * L + slot] of frame
// frm[pair] (side 0), cell j = mj[..] of frame frm[P + pair] (side 1).  Window token t =
// (dy, dx) of side s reads fine pixel (stride r - 2 + dy, stride c - 2 + dx) (zero
// outside, F.unfold padding 2) -> bf16 win[((s * M + m) * 25 + t)][128]; the matched
// coarse rows (side-major coarse residual stream xc) -> bf16 crow[s * M + m][256].
__global__ void k_lf_windows(const float* __restrict__ fine, int Hf, int Wf, int wc, int stride,
                             const int32_t* __restrict__ frm, int P, const int32_t* __restrict__ mi,
                             const int32_t* __restrict__ mj, int L, const int32_t* __restrict__ mp,
                             const int32_t* __restrict__ ms, int M, const float* __restrict__ xc,
                             bf16_t* __restrict__ win, bf16_t* __restrict__ crow) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nwin = (long)2 * M * 25 * 32;  // (side, m, t, c4) over 32 c4
    if (e < nwin) {
        const int c4 = (int)(e % 32);
        long r = e / 32;
        const int t = (int)(r % 25);
        const long sm = r / 25;
        const int m = (int)(sm % M), side = (int)(sm / M);
        const int p = mp[m];
        const size_t o = (size_t)p * L + ms[m];
        const int cell = side ? mj[o] : mi[o], frame = frm[side * P + p];
        const int y = (cell / wc) * stride - 2 + t / 5, x = (cell % wc) * stride - 2 + t % 5;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < Hf && x >= 0 && x < Wf)
            v = reinterpret_cast<const float4*>(fine + (((size_t)frame * Hf + y) * Wf + x) * 128)[c4];
        reinterpret_cast<uint2*>(win + (size_t)r * 128)[c4] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
        return;
    }
    const long e2 = e - nwin;  // coarse rows: (side, m, c4) over 64 c4
    if (e2 >= (long)2 * M * 64) return;
    const int c4 = (int)(e2 % 64);
    const long r = e2 / 64;
    const int m = (int)(r % M), side = (int)(r / M);
    const int p = mp[m];
    const size_t o = (size_t)p * L + ms[m];
    const size_t src = ((size_t)side * P + p) * L + (side ? mj[o] : mi[o]);
    const float4 v = reinterpret_cast<const float4*>(xc + src * 256)[c4];
    reinterpret_cast<uint2*>(crow + (size_t)r * 256)[c4] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}

// x[(s, m, t)][c] = A[(s, m, t)][c] + Cm[(s, m)][c] (f32) and its bf16 copy into cat
__global__ void k_lf_fine_tokens(const float* __restrict__ A, const float* __restrict__ Cm, long rows,
                                 float* __restrict__ x, bf16_t* __restrict__ cat) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (row, c4) over 32
    if (e >= rows * 32) return;
    const long row = e / 32;
    const int c4 = (int)(e % 32);
    const float4 a = reinterpret_cast<const float4*>(A + row * 128)[c4];
    const float4 c = reinterpret_cast<const float4*>(Cm + (row / 25) * 128)[c4];
    const float4 y = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    reinterpret_cast<float4*>(x + row * 128)[c4] = y;
    reinterpret_cast<uint2*>(cat + row * 256)[c4] = make_uint2(pack_bf16x2(y.x, y.y), pack_bf16x2(y.z, y.w));
}

// per match: heatmap = softmax(x0[m][12] . x1[m][r] * 128^-1/2); expectation on the
// normalised grid (x = linspace(-1, 1, 5)[r % 5], y = [r / 5]); keypoints in pixels:
// kpts0 = 8 (i % wc, i / wc), kpts1 = 8 (j % wc, j / wc) + 2 * 2 * (x, y)
__global__ __launch_bounds__(64) void k_lf_fine_match(const float* __restrict__ xf, int M,
                                                      const int32_t* __restrict__ mp, const int32_t* __restrict__ ms,
                                                      const int32_t* __restrict__ mi, const int32_t* __restrict__ mj,
                                                      const float* __restrict__ mconf, int L, int wc, float scale_c,
                                                      float scale_f, float* __restrict__ kp0, float* __restrict__ kp1,
                                                      float* __restrict__ conf) {
    const int m = blockIdx.x, lane = threadIdx.x;
    if (m >= M) return;
    const float* c0 = xf + ((size_t)m * 25 + 12) * 128;
    float sim = -INFINITY;
    if (lane < 25) {
        const float* w = xf + (((size_t)M + m) * 25 + lane) * 128;
        float a = 0.f;
        for (int c = 0; c < 128; ++c) a = fmaf(c0[c], w[c], a);
        sim = 0.08838834764831845f * a;
    }
    const float mx = wave_max(sim);
    const float ex = lane < 25 ? expf(sim - mx) : 0.f;
    const float z = wave_sum(ex);
    const float h = ex / z;
    const float g = lane < 25 ? -1.f + 0.5f * (float)(lane % 5) : 0.f;
    const float gy = lane < 25 ? -1.f + 0.5f * (float)(lane / 5) : 0.f;
    const float cx = wave_sum(h * g), cy = wave_sum(h * gy);
    if (lane == 0) {
        const size_t o = (size_t)mp[m] * L + ms[m];
        const int i = mi[o], j = mj[o];
        kp0[2 * o] = (float)(i % wc) * scale_c;
        kp0[2 * o + 1] = (float)(i / wc) * scale_c;
        kp1[2 * o] = (float)(j % wc) * scale_c + cx * 2.0f * scale_f;
        kp1[2 * o + 1] = (float)(j / wc) * scale_c + cy * 2.0f * scale_f;
        conf[o] = mconf[o];
    }
}

struct FeatBufs {
    float* xf;     // residual stream f32 (up to 256 channels)
    bf16_t* xb;    // its bf16 copy
    bf16_t* yb;    // block-internal bf16 activation
    float* rf;     // shortcut / lateral f32
    float* tf;     // FPN f32 temporaries
    bf16_t* zero;  // zero bytes: the convs' padding taps
    float* c2;     // layer2 output f32 (1/4) kept for the FPN
    uint8_t* gray; // resized gray frames (H, W not multiples of 8)
};

size_t feat_carve(int B, int H, int W, void* base, FeatBufs* out) {
    const size_t P2 = (size_t)B * (H / 2) * (W / 2);  // 1/2-resolution pixels
    WsCarver c(base);
    FeatBufs b;
    b.xf = c.take<float>(P2 * 256);
    b.xb = c.take<bf16_t>(P2 * 256);
    b.yb = c.take<bf16_t>(P2 * 256);
    b.rf = c.take<float>(P2 * 256);
    b.tf = c.take<float>(P2 * 256);
    b.zero = c.take<bf16_t>(128);
    c.take<float>(P2 / 16 * 256 + 64);  // layer3 output f32 (1/8): no longer used, the size stays
    b.c2 = c.take<float>(P2 / 4 * 256 + 64);
    b.gray = c.take<uint8_t>(P2 * 4);
    if (out) *out = b;
    return c.total();
}

int conv(const mlg_loftr_weights& w, int idx, const bf16_t* in, int B, int H, int W, const bf16_t* zero,
         const float* R, float* X, bf16_t* C, int act, hipStream_t s) {
    const ConvSpec sp = CONVS[idx];
    if (sp.k != 1 || sp.s != 1)  // 3x3 and strided 1x1: implicit GEMM (no patch matrix)
        return mlg_conv_implicit(in, zero, B, H, W, sp.cin, sp.k, sp.s, (const bf16_t*)w.conv_w[idx], w.conv_b[idx],
                                 R, sp.cout, X, sp.cout, C, sp.cout, act, sp.cout, sp.cout, s);
    const long M = (long)B * H * W;
    return mlg_gemm_conv(in, sp.cin, (const bf16_t*)w.conv_w[idx], w.conv_b[idx], R, sp.cout, X, sp.cout, C, sp.cout,
                         act, sp.cout, (int)M, sp.cout, sp.cin, s);
}

// one BasicBlock: in (f32 x + bf16 xb) -> out (same buffers), stride 1 or 2
int basic_block(const mlg_loftr_weights& w, int c1, int c2, int cds, int B, int H, int W, float* x, bf16_t* xb,
                bf16_t* yb, float* rf, const bf16_t* zero, hipStream_t s) {
    const int st = CONVS[c1].s, Ho = (H + st - 1) / st, Wo = (W + st - 1) / st;
    MLG_TRY(conv(w, c1, xb, B, H, W, zero, nullptr, nullptr, yb, 1, s));  // relu(bn1(conv1 x))
    const float* R = x;
    if (cds >= 0) {  // bn(downsample x) -> rf
        MLG_TRY(conv(w, cds, xb, B, H, W, zero, nullptr, rf, nullptr, 0, s));
        R = rf;
    }
    // relu(R + bn2(conv2 y)) -> x (f32) + xb; R may alias x (stride 1: same shape)
    return conv(w, c2, yb, B, Ho, Wo, zero, R, x, xb, 1, s);
}

// FPN merge: bf16(outconv(x) + up2x(coarser)) -> out.  MLG_LF_FPN_FUSED=1: the
// upsample-add in the lateral 1x1 conv's epilogue (EpiConvUp, gemm_bf16.hip; no f32
// lateral map written and re-read): backbone -3 % in a same-box A/B and the LoFTR GPU tests
// pass, but its features are not bit-identical to this two-kernel form for a reason not yet
// found (profiles/r06y_ab_loftr_fpn_fused.txt), so it stays off; default: the conv's f32
// output to `tf`, then k_lf_up_add.
#ifndef MLG_LF_FPN_FUSED
#define MLG_LF_FPN_FUSED 0
#endif
int fpn_merge(const mlg_loftr_weights& w, int idx, const bf16_t* in, int B, int H, int W, const float* coarser,
              float* tf, bf16_t* out, hipStream_t s) {
    const ConvSpec sp = CONVS[idx];
    if (sp.k != 1 || sp.s != 1 || (H % 2) || (W % 2)) return MLG_EINVAL;
    if (MLG_LF_FPN_FUSED)
        return mlg_gemm_conv_upadd(in, sp.cin, (const bf16_t*)w.conv_w[idx], w.conv_b[idx], coarser, H / 2, W / 2, out,
                                   B * H * W, sp.cout, sp.cin, s);
    MLG_TRY(conv(w, idx, in, B, H, W, nullptr, nullptr, tf, nullptr, 0, s));
    const long n = (long)B * H * W * (sp.cout / 4);
    hipLaunchKernelGGL(k_lf_up_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tf, coarser, B, H / 2, W / 2,
                       sp.cout, out);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

}  // namespace

size_t mlg_loftr_features_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H < 32 || W < 32) return 0;
    return feat_carve(B, H / 8 * 8, W / 8 * 8, nullptr, nullptr);
}

int mlg_loftr_features(const mlg_loftr_weights* wp, const uint8_t* frames_in, int B, int H_in, int W_in, int C,
                       long frame_stride, void* ws, size_t ws_bytes, float* coarse, float* fine, void* stream) {
    if (!mlg_head_ok(wp, MLG_ABI_VERSION) || !frames_in || !ws || !coarse || !fine || B <= 0 || H_in < 32 || W_in < 32 ||
        (C != 1 && C != 3 && C != 4))
        return MLG_EINVAL;
    const int H = H_in / 8 * 8, W = W_in / 8 * 8;
    FeatBufs b;
    if (feat_carve(B, H, W, ws, &b) > ws_bytes) return MLG_ENOMEM;
    const uint8_t* frames = frames_in;
    if (H != H_in || W != W_in) {  // cv2 gray + INTER_LINEAR resize to multiples of 8
        int vend = 0;  // first byte of a row in the vertical pass's scalar tail
        for (; vend <= W - 16; vend += 16) {}
        for (; vend < W - 8; vend += 8) {}
        uint8_t* g = b.gray;
        const long n = (long)B * H * W;
        hipLaunchKernelGGL(k_lf_gray_resize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           frames_in, frame_stride, H_in, W_in, C, H, W, vend, g, B);
        MLG_LAUNCH_CHECK();
        frames = g;
        C = 1;
        frame_stride = (long)H * W;
    }
    const mlg_loftr_weights& w = *wp;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(b.zero, 0, 256, (hipStream_t)stream) != hipSuccess) return MLG_EHIP;
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
    hipLaunchKernelGGL(k_lf_stem, dim3((W2 + 15) / 16, (H2 + 7) / 8, B), dim3(256), 0, s, frames, frame_stride, H, W,
                       C, w.stem_w, w.stem_b, b.xf, b.xb);
    MLG_LAUNCH_CHECK();
    // layer1 (1/2, 128)
    MLG_TRY(basic_block(w, 0, 1, -1, B, H2, W2, b.xf, b.xb, b.yb, b.rf, b.zero, s));
    MLG_TRY(basic_block(w, 2, 3, -1, B, H2, W2, b.xf, b.xb, b.yb, b.rf, b.zero, s));
    // x1 (bf16) is needed by the FPN: kept in `fine` (scratch until the end: fine is
    // written last)
    bf16_t* x1b = (bf16_t*)fine;
    if (hipMemcpyAsync(x1b, b.xb, (size_t)B * H2 * W2 * 128 * 2, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return MLG_EHIP;
    // layer2 (1/4, 256p)
    MLG_TRY(basic_block(w, 4, 5, 6, B, H2, W2, b.xf, b.xb, b.yb, b.rf, b.zero, s));
    MLG_TRY(basic_block(w, 7, 8, -1, B, H4, W4, b.xf, b.xb, b.yb, b.rf, b.zero, s));
    bf16_t* x2b = (bf16_t*)b.c2;  // bf16 copy of x2 (b.c2 is free until the FPN needs its f32 slot)
    if (hipMemcpyAsync(x2b, b.xb, (size_t)B * H4 * W4 * 256 * 2, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return MLG_EHIP;
    // layer3 (1/8, 256)
    MLG_TRY(basic_block(w, 9, 10, 11, B, H4, W4, b.xf, b.xb, b.yb, b.rf, b.zero, s));
    MLG_TRY(basic_block(w, 12, 13, -1, B, H8, W8, b.xf, b.xb, b.yb, b.rf, b.zero, s));
    // FPN: x3_out = outconv3(x3) -> coarse output (f32)
    MLG_TRY(conv(w, 14, b.xb, B, H8, W8, b.zero, nullptr, coarse, nullptr, 0, s));
    // x2_out = outconv2(x2) + up(x3_out) -> bf16 -> conv + BN + leaky -> conv
    MLG_TRY(fpn_merge(w, 15, x2b, B, H4, W4, coarse, b.tf, b.yb, s));
    MLG_TRY(conv(w, 16, b.yb, B, H4, W4, b.zero, nullptr, nullptr, b.xb, 2, s));
    MLG_TRY(conv(w, 17, b.xb, B, H4, W4, b.zero, nullptr, b.c2, nullptr, 0, s));  // x2_out f32 (1/4, 256p)
    // x1_out = outconv1(x1) + up(x2_out) -> conv + BN + leaky -> conv -> fine
    MLG_TRY(fpn_merge(w, 18, x1b, B, H2, W2, b.c2, b.tf, b.yb, s));
    MLG_TRY(conv(w, 19, b.yb, B, H2, W2, b.zero, nullptr, nullptr, b.xb, 2, s));
    MLG_TRY(conv(w, 20, b.xb, B, H2, W2, b.zero, nullptr, fine, nullptr, 0, s));
    return MLG_OK;
}

// ------------------------------------------------------------- matching -----
namespace {

// Coarse layers' block tail (merge, norm1, MLP, norm2, residual) as ONE fused kernel per
// 64-token tile (lg_ffn.hip, LoFTR form): the merge output, the MLP hidden and the
// pre-norm2 message never leave LDS (per token 3.5 KB of HBM instead of ~11 KB through
// five launches).  The unfused GEMM + LayerNorm sequence stays reachable at run time
// (mlg_op_loftr_coarse_layer, fused = 0).
// Coarse similarity f0 . f1^T from split-bf16 operands (hi * hi + hi * lo + lo * hi, f32
// accumulation: products to ~2^-17 of f32) instead of the exact-f32 MFMA
int g_lf_sim_split = 1;  // mlg_set_loftr_similarity
// The split similarity of a dual-softmax group is ONE persistent GEMM launch (round 6): per
// pair, 576 tiles (720 x 536) or 361 (640 x 480) over 256 workgroups left a 2-3-tile tail
// (-3.5 % matching, bit-identical, profiles/r06o_ab_loftr_sim_batched.txt).
// Layer 0 (self) runs once per distinct frame of the call, its rows gathered per pair side
// (round 6: -4 % matching per pair, profiles/r06x_ab_loftr_self0_dedup.txt).  Row-independent
// kernels: same bits (tests/test_loftr_gpu.py pins the equality).

// nn.Linear weight [N][K] bf16 -> k-step-major [K / 16][N][16] (lg_ffn.hip's layout)
__global__ void k_lf_pack_kstep(const bf16_t* __restrict__ w, int N, int K, bf16_t* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * K) return;
    const int n = (int)(i / K), k = (int)(i % K);
    out[((size_t)(k >> 4) * N + n) * 16 + (k & 15)] = w[i];
}

struct TailW {  // one coarse layer's packed block-tail weights (workspace)
    bf16_t *wmerge, *w1, *w2;
    float *ln_g, *ln_b;  // [norm1 | norm2]
};
constexpr size_t TAIL_ELEMS = 256 * 256 + 512 * 512 + 256 * 512;  // bf16 per layer

struct LayerBufs {
    float* x;     // [rows][d] residual stream
    bf16_t* cat;  // [rows][2d]: bf16(x) | norm1(msg)
    float* qkv;   // [rows][3d]
    bf16_t* msg;  // [rows][d]
    float* t;     // [rows][d]
    bf16_t* h;    // [rows][2d]
    float* kv;    // [segs][8][dh][dh]
    float* ks;    // [segs][8][dh]
    float* kvp;   // [segs][8][chunks][dh * dh + dh] partial sums (segments > LF_KV_CHUNK tokens)
};

// One LoFTREncoderLayer over `nseg` segments of L tokens (rows x0 .. of the buffers);
// source rows src0 (== x0 for self).  d = 256 (coarse) or 128 (fine).
int encoder_layer(const mlg_loftr_layer& lw, const LayerBufs& b, int d, long x0, long src0, int nseg, int L,
                  hipStream_t s, const TailW* tw = nullptr) {
    const long rows = (long)nseg * L;
    const int dh = d / 8;
    float* qkv = b.qkv + x0 * 3 * d;
    // q | k | v, elu + 1 on q and k, v stored as v / L (the reference's values / v_length,
    // divided once here rather than per (k, v) product in k_lf_kv*)
    const float vl = (float)L;
    if (x0 == src0) {
        MLG_TRY(mlg_gemm_conv(b.cat + x0 * 2 * d, 2 * d, (const bf16_t*)lw.w, nullptr, nullptr, 0, qkv, 3 * d, nullptr,
                             0, 3, 2 * d, (int)rows, 3 * d, d, s, vl));
    } else {
        MLG_TRY(mlg_gemm_conv(b.cat + x0 * 2 * d, 2 * d, (const bf16_t*)lw.w, nullptr, nullptr, 0, qkv, 3 * d, nullptr,
                             0, 3, d, (int)rows, d, d, s));
        MLG_TRY(mlg_gemm_conv(b.cat + src0 * 2 * d, 2 * d, (const bf16_t*)lw.w + (size_t)d * d, nullptr, nullptr, 0,
                             qkv + d, 3 * d, nullptr, 0, 3, d, (int)rows, 2 * d, d, s, vl));
    }
    float* kv = b.kv + (size_t)(x0 / L) * 8 * dh * dh;
    float* ks = b.ks + (size_t)(x0 / L) * 8 * dh;
    const int nch = (L + LF_KV_CHUNK - 1) / LF_KV_CHUNK;
    const unsigned apply_blocks = (unsigned)(((long)nseg * ((L + 63) / 64) * 8 + 3) / 4);
    if (d == 256) {
        if (nch > 1) {  // long segments: chunked partial sums, combined in chunk order
            hipLaunchKernelGGL(k_lf_kv_part<32>, dim3((unsigned)((nseg * 8 * nch + 3) / 4)), dim3(256), 0, s, qkv + d,
                               qkv + 2 * d, 3 * d, 3 * d, L, 8, nseg, nch, b.kvp);
            MLG_LAUNCH_CHECK();
            const long items = (long)nseg * 8 * (32 * 32 + 32);
            hipLaunchKernelGGL(k_lf_kv_combine<32>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, b.kvp,
                               nseg * 8, nch, kv, ks);
        } else {
            hipLaunchKernelGGL(k_lf_kv<32>, dim3(nseg * 8), dim3(256), 0, s, qkv + d, qkv + 2 * d, 3 * d, 3 * d, L, 8,
                               (const int32_t*)nullptr, kv, ks);
        }
        MLG_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_lf_apply<32>, dim3(apply_blocks), dim3(256), 0, s, qkv, 3 * d, kv, ks, L, 8, nseg,
                           b.msg + x0 * d);
    } else {
        if (nch > 1) {
            hipLaunchKernelGGL(k_lf_kv_part<16>, dim3((unsigned)((nseg * 8 * nch + 3) / 4)), dim3(256), 0, s, qkv + d,
                               qkv + 2 * d, 3 * d, 3 * d, L, 8, nseg, nch, b.kvp);
            MLG_LAUNCH_CHECK();
            const long items = (long)nseg * 8 * (16 * 16 + 16);
            hipLaunchKernelGGL(k_lf_kv_combine<16>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, b.kvp,
                               nseg * 8, nch, kv, ks);
        } else {
            hipLaunchKernelGGL(k_lf_kv<16>, dim3(nseg * 8), dim3(256), 0, s, qkv + d, qkv + 2 * d, 3 * d, 3 * d, L, 8,
                               (const int32_t*)nullptr, kv, ks);
        }
        MLG_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_lf_apply<16>, dim3(apply_blocks), dim3(256), 0, s, qkv, 3 * d, kv, ks, L, 8, nseg,
                           b.msg + x0 * d);
    }
    MLG_LAUNCH_CHECK();
    if (tw) {  // d == 256: merge -> norm1 -> MLP -> norm2 -> residual, fused
        mlg_lg_block bw{};
        bw.Wout = tw->wmerge;
        bw.Wf1 = tw->w1;
        bw.Wf2 = tw->w2;
        bw.ln_g = tw->ln_g;
        bw.ln_b = tw->ln_b;
        return mlg_lg_ffn(b.msg + x0 * d, b.x + x0 * d, b.cat + x0 * 2 * d, 2 * d, (int)rows, bw, s, nullptr, 2);
    }
    // merge -> norm1 -> bf16 into cat[:, d:]
    MLG_TRY(mlg_gemm_conv(b.msg + x0 * d, d, (const bf16_t*)lw.wmerge, nullptr, nullptr, 0, b.t + x0 * d, d, nullptr,
                         0, 0, 0, (int)rows, d, d, s));
    const unsigned lnb = (unsigned)((rows + 3) / 4);
    if (d == 256)
        hipLaunchKernelGGL(k_lf_ln<256>, dim3(lnb), dim3(256), 0, s, b.t + x0 * d, lw.ln1_g, lw.ln1_b, rows, 0,
                           (float*)nullptr, b.cat + x0 * 2 * d + d, 2 * d);
    else
        hipLaunchKernelGGL(k_lf_ln<128>, dim3(lnb), dim3(256), 0, s, b.t + x0 * d, lw.ln1_g, lw.ln1_b, rows, 0,
                           (float*)nullptr, b.cat + x0 * 2 * d + d, 2 * d);
    MLG_LAUNCH_CHECK();
    // MLP: relu([x | msg] W1^T) W2^T -> norm2 -> residual
    MLG_TRY(mlg_gemm_conv(b.cat + x0 * 2 * d, 2 * d, (const bf16_t*)lw.w1, nullptr, nullptr, 0, nullptr, 0,
                         b.h + x0 * 2 * d, 2 * d, 1, 2 * d, (int)rows, 2 * d, 2 * d, s));
    MLG_TRY(mlg_gemm_conv(b.h + x0 * 2 * d, 2 * d, (const bf16_t*)lw.w2, nullptr, nullptr, 0, b.t + x0 * d, d, nullptr,
                         0, 0, 0, (int)rows, d, 2 * d, s));
    if (d == 256)
        hipLaunchKernelGGL(k_lf_ln<256>, dim3(lnb), dim3(256), 0, s, b.t + x0 * d, lw.ln2_g, lw.ln2_b, rows, 1,
                           b.x + x0 * d, b.cat + x0 * 2 * d, 2 * d);
    else
        hipLaunchKernelGGL(k_lf_ln<128>, dim3(lnb), dim3(256), 0, s, b.t + x0 * d, lw.ln2_g, lw.ln2_b, rows, 1,
                           b.x + x0 * d, b.cat + x0 * 2 * d, 2 * d);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

// the reference's layer order: self on both sides; cross updates side 0 from side 1,
// then side 1 from the updated side 0.  Side-major rows: side s, segment g at
// (s * nseg + g) * L.
int transformer(const mlg_loftr_layer* layers, int nl, const LayerBufs& b, int d, int nseg, int L, hipStream_t s,
                const TailW* tails = nullptr, int first = 0) {
    const long half = (long)nseg * L;
    for (int i = first; i < nl; ++i) {
        const TailW* tw = tails ? tails + i : nullptr;
        if (i % 2 == 0) {
            MLG_TRY(encoder_layer(layers[i], b, d, 0, 0, 2 * nseg, L, s, tw));
        } else {
            MLG_TRY(encoder_layer(layers[i], b, d, 0, half, nseg, L, s, tw));
            MLG_TRY(encoder_layer(layers[i], b, d, half, 0, nseg, L, s, tw));
        }
    }
    return MLG_OK;
}

constexpr size_t TAILS_BYTES = (size_t)8 * TAIL_ELEMS * 2 + (size_t)8 * 1024 * 4;

// where each coarse layer's packed tail weights live in a TAILS_BYTES buffer
void tails_at(char* base, TailW (&tw)[8]) {
    bf16_t* p = (bf16_t*)base;
    float* f = (float*)(base + 8 * TAIL_ELEMS * 2);
    for (int l = 0; l < 8; ++l) {
        tw[l].wmerge = p;
        tw[l].w1 = p + 256 * 256;
        tw[l].w2 = p + 256 * 256 + 512 * 512;
        tw[l].ln_g = f + l * 1024;
        tw[l].ln_b = f + l * 1024 + 512;
        p += TAIL_ELEMS;
    }
}

// the coarse layers' tail weights packed for the fused kernel (24 small launches + 32
// copies: once per weights via mlg_loftr_pack_tails, or per call into the workspace)
int pack_tails(const mlg_loftr_weights& w, char* base, TailW (&tw)[8], hipStream_t s) {
    tails_at(base, tw);
    for (int l = 0; l < 8; ++l) {
        const mlg_loftr_layer& lw = w.coarse[l];
        const struct { const uint16_t* src; bf16_t* dst; int n, k; } m[3] = {
            {lw.wmerge, tw[l].wmerge, 256, 256}, {lw.w1, tw[l].w1, 512, 512}, {lw.w2, tw[l].w2, 256, 512}};
        for (const auto& e : m) {
            const long n = (long)e.n * e.k;
            hipLaunchKernelGGL(k_lf_pack_kstep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                               (const bf16_t*)e.src, e.n, e.k, e.dst);
            MLG_LAUNCH_CHECK();
        }
        if (hipMemcpyAsync(tw[l].ln_g, lw.ln1_g, 1024, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(tw[l].ln_g + 256, lw.ln2_g, 1024, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(tw[l].ln_b, lw.ln1_b, 1024, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(tw[l].ln_b + 256, lw.ln2_b, 1024, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return MLG_EHIP;
    }
    return MLG_OK;
}

// a transformer's scratch behind its token buffers x / cat (rows tokens of width d, nseg
// segments of L tokens each; kvp: with the chunked K^T V partial sums)
void layer_carve(WsCarver& c, size_t rows, size_t nseg, int L, int d, bool kvp, LayerBufs* b) {
    const size_t dh = (size_t)d / 8;
    b->qkv = c.take<float>(rows * 3 * d);
    b->msg = c.take<bf16_t>(rows * d);
    b->t = c.take<float>(rows * d);
    b->h = c.take<bf16_t>(rows * 2 * d);
    b->kv = c.take<float>(nseg * 8 * dh * dh);
    b->ks = c.take<float>(nseg * 8 * dh);
    b->kvp = kvp ? c.take<float>(nseg * 8 * ((L + LF_KV_CHUNK - 1) / LF_KV_CHUNK) * (dh * dh + dh)) : nullptr;
}

constexpr int FINE_CHUNK = 4096;  // matches per fine-stage pass

struct MatchBufs {
    LayerBufs bc;  // coarse transformer (rows 2 P L, d 256)
    LayerBufs bf;  // fine transformer (rows 2 C 25, d 128)
    bf16_t *win, *crow, *cd;
    float *cm, *S;
    bf16_t* csplit;
    float *rmax, *rsum, *rkey, *cmax, *csum, *ckey, *pm, *pz, *prm, *bval;
    int32_t* bidx;
    float* cbest;
    int32_t *mi, *mj;
    float* mconf;
    int32_t *cnt, *frm, *ufr, *umap, *mp, *ms;
    char* tails;
};

size_t match_carve(int P, int L, void* base, MatchBufs* out) {
    WsCarver c(base);
    MatchBufs M;
    const size_t rc = (size_t)2 * P * L, rf = (size_t)2 * FINE_CHUNK * 25;
    M.bc.x = c.take<float>(rc * 256);
    M.bc.cat = c.take<bf16_t>(rc * 512);
    layer_carve(c, rc, (size_t)2 * P, L, 256, true, &M.bc);
    M.bf.x = c.take<float>(rf * 128);
    M.bf.cat = c.take<bf16_t>(rf * 256);
    layer_carve(c, rf, (size_t)2 * FINE_CHUNK, 25, 128, false, &M.bf);
    M.win = c.take<bf16_t>(rf * 128);
    M.crow = c.take<bf16_t>((size_t)2 * FINE_CHUNK * 256);
    M.cd = c.take<bf16_t>((size_t)2 * FINE_CHUNK * 128);
    M.cm = c.take<float>((size_t)2 * FINE_CHUNK * 128);
    const size_t G = (size_t)std::min(P, MLG_LF_PGRP);  // pairs per dual-softmax group
    const size_t Lp = (size_t)(L + 3) / 4 * 4;          // S / ckey row stride (split path)
    M.S = c.take<float>(G * L * Lp);
    // the coarse features as split-bf16 rows [hi | lo] (+ 256 zero rows: the similarity
    // GEMM reads B rows up to its 256-column tile), in the q / k / v buffer, which the
    // coarse transformer no longer needs when the similarity runs (3x larger: 2 P L x 768 f32)
    const size_t csplit_elems = (rc + 256) * 512;
    M.csplit = csplit_elems * sizeof(bf16_t) <= rc * 768 * sizeof(float) ? (bf16_t*)M.bc.qkv
                                                                         : c.take<bf16_t>(csplit_elems);
    M.rmax = c.take<float>(G * L);
    M.rsum = c.take<float>(G * L);
    M.rkey = c.take<float>(G * L);
    M.cmax = c.take<float>(G * L);
    M.csum = c.take<float>(G * L);
    M.ckey = c.take<float>(G * Lp);
    const size_t nrch = (size_t)(L + LF_RCH - 1) / LF_RCH;
    M.pm = c.take<float>(G * nrch * L);
    M.pz = c.take<float>(G * nrch * L);
    M.prm = c.take<float>(G * ((L + 255) / 256) * L);
    M.bval = c.take<float>(G * L);
    M.bidx = c.take<int32_t>(G * L);
    M.cbest = c.take<float>(G * L);
    M.mi = c.take<int32_t>((size_t)P * L);
    M.mj = c.take<int32_t>((size_t)P * L);
    M.mconf = c.take<float>((size_t)P * L);
    M.cnt = c.take<int32_t>((size_t)P);
    M.frm = c.take<int32_t>((size_t)2 * P);
    M.ufr = c.take<int32_t>((size_t)2 * P);
    M.umap = c.take<int32_t>((size_t)2 * P);
    M.mp = c.take<int32_t>((size_t)FINE_CHUNK);
    M.ms = c.take<int32_t>((size_t)FINE_CHUNK);
    M.tails = c.take<char>(TAILS_BYTES);
    if (out) *out = M;
    return c.total();
}

}  // namespace

size_t mlg_loftr_match_ws_bytes(int P, int H, int W) {
    if (P <= 0 || H < 32 || W < 32 || (H % 8) || (W % 8)) return 0;
    return match_carve(P, (H / 8) * (W / 8), nullptr, nullptr);
}

int mlg_loftr_match(const mlg_loftr_weights* wp, const float* coarse, const float* fine, int H, int W,
                    const int32_t* pa, const int32_t* pb, int P, const float* pe, void* ws, size_t ws_bytes,
                    int32_t* counts, float* kpts0, float* kpts1, float* conf, void* stream) {
    if (!mlg_head_ok(wp, MLG_ABI_VERSION) || !coarse || !fine || !pa || !pb || !pe || !ws || !counts || !kpts0 || !kpts1 || !conf || P <= 0 ||
        H < 32 || W < 32 || (H % 8) || (W % 8))
        return MLG_EINVAL;
    const int hc = H / 8, wc = W / 8, L = hc * wc, Hf = H / 2, Wf = W / 2;
    MatchBufs b;
    if (match_carve(P, L, ws, &b) > ws_bytes) return MLG_ENOMEM;
    const mlg_loftr_weights& w = *wp;
    hipStream_t s = (hipStream_t)stream;
    const LayerBufs &bc = b.bc, &bf = b.bf;
    const int nrch = (L + LF_RCH - 1) / LF_RCH, ncb = (L + 255) / 256;

    // coarse tokens, side-major: side 0 = frames pa, side 1 = frames pb
    std::vector<int32_t> h_frames(2 * P);
    for (int p = 0; p < P; ++p) {
        h_frames[p] = pa[p];
        h_frames[P + p] = pb[p];
    }
    if (hipMemcpyAsync(b.frm, h_frames.data(), h_frames.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess)
        return MLG_EHIP;
    const long crows = (long)2 * P * L;
    TailW tails[8];
    if (w.coarse_tails)
        tails_at((char*)w.coarse_tails, tails);  // packed once (mlg_loftr_pack_tails)
    else
        MLG_TRY(pack_tails(w, b.tails, tails, s));
    const TailW* tw = tails;
    // the distinct frames of the call (first-appearance order) and each pair side's index
    const pair_plan::Distinct uf = pair_plan::distinct_frames(h_frames.data(), h_frames.size());
    const std::vector<int32_t>& h_ufr = uf.unique;
    const std::vector<int32_t>& h_umap = uf.index;
    const int NU = (int)h_ufr.size();
    if (NU < 2 * P) {
        if (hipMemcpyAsync(b.ufr, h_ufr.data(), (size_t)NU * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(b.umap, h_umap.data(), (size_t)2 * P * 4, hipMemcpyHostToDevice, s) != hipSuccess)
            return MLG_EHIP;
        const long urows = (long)NU * L;
        hipLaunchKernelGGL(k_lf_tokens, dim3((unsigned)((urows * 64 + 255) / 256)), dim3(256), 0, s, coarse, b.ufr, L,
                           pe, bc.x, bc.cat, (int)urows);
        MLG_LAUNCH_CHECK();
        MLG_TRY(encoder_layer(w.coarse[0], bc, 256, 0, 0, NU, L, s, tw));
        // the NU frames' rows aside in the dead q / k / v buffer (2 P L x 3 KiB >= NU L x
        // 1.5 KiB), then laid out per pair side
        float* tx = bc.qkv;
        bf16_t* tc = (bf16_t*)(bc.qkv + urows * 256);
        hipLaunchKernelGGL(k_lf_stash, dim3((unsigned)((urows * 96 + 255) / 256)), dim3(256), 0, s, bc.x, bc.cat,
                           urows, tx, tc);
        MLG_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_lf_gather_rows, dim3((unsigned)((crows * 96 + 255) / 256)), dim3(256), 0, s, tx, tc,
                           b.umap, L, crows, bc.x, bc.cat);
        MLG_LAUNCH_CHECK();
        MLG_TRY(transformer(w.coarse, 8, bc, 256, P, L, s, tw, 1));
    } else {
        hipLaunchKernelGGL(k_lf_tokens, dim3((unsigned)((crows * 64 + 255) / 256)), dim3(256), 0, s, coarse, b.frm, L,
                           pe, bc.x, bc.cat, (int)crows);
        MLG_LAUNCH_CHECK();
        MLG_TRY(transformer(w.coarse, 8, bc, 256, P, L, s, tw));
    }
    // the coarse similarity: split-bf16 operands (3 bf16 MFMA products at ~6x the exact-f32
    // MFMA's rate) or the exact-f32 MFMA (mlg_set_loftr_similarity(1)).  The split GEMM
    // writes 16-B row pieces, so its S rows are lds = L rounded up to 4 floats, the pad
    // columns -inf (EpiSimLoFTR): frames of L % 4 != 0 cells -- the ISEC 720 x 536, L =
    // 6030 -- take the split path too (round 6; before, the exact-f32 one)
    bf16_t* const CS = b.csplit;
    const int Lpad = (L + 255) / 256 * 256;
    const bool split = g_lf_sim_split != 0;
    const int lds = split ? (L + 3) / 4 * 4 : L;
    if (split) {
        const long rows = (long)2 * P * L;
        hipLaunchKernelGGL(k_lf_split_rows, dim3((unsigned)((rows * 64 + 255) / 256)), dim3(256), 0, s, bc.x, rows, CS);
        MLG_LAUNCH_CHECK();
        if (hipMemsetAsync(CS + (size_t)rows * 512, 0, (size_t)256 * 512 * 2, s) != hipSuccess) return MLG_EHIP;
    }
    // dual softmax + mutual nearest, MLG_LF_PGRP pairs at a time over [G][L][L] similarity
    const int G = std::min(P, MLG_LF_PGRP);
    for (int p0 = 0; p0 < P; p0 += G) {
        const unsigned g = (unsigned)std::min(G, P - p0);
        if (split) {  // the group's g similarities as one tile queue
            MLG_TRY(mlg_gemm_sim_split_loftr(CS + (size_t)p0 * L * 512, CS + ((size_t)P + p0) * L * 512, L, Lpad, 256,
                                            b.S, lds, L, s, (int)g, (long)L * 512));
        } else {
            for (int q = 0; q < (int)g; ++q) {
                const int p = p0 + q;
                MLG_TRY(mlg_similarity_f32_loftr(bc.x + (size_t)p * L * 256, L, bc.x + ((size_t)P + p) * L * 256, L, 256,
                                                b.S + (size_t)q * L * lds, L, s));
            }
        }
        // three reads of S: stats, rowbest, colmaxpart
        hipLaunchKernelGGL(k_lf_stats, dim3(ncb, nrch, g), dim3(256), 0, s, b.S, L, lds, b.pm, b.pz, b.prm);
        hipLaunchKernelGGL(k_lf_colfin, dim3((L + 63) / 64, 1, g), dim3(256), 0, s, b.pm, b.pz, L, lds, nrch, b.cmax,
                           b.csum, b.ckey);
        hipLaunchKernelGGL(k_lf_rowbest, dim3((L + 3) / 4, 1, g), dim3(256), 0, s, b.S, L, lds, b.rmax, b.rsum, b.rkey,
                           b.prm, ncb, b.cmax, b.csum, b.ckey, b.bval, b.bidx);
        hipLaunchKernelGGL(k_lf_colmaxpart, dim3((L + 255) / 256, nrch, g), dim3(256), 0, s, b.S, L, lds, b.rmax,
                           b.rsum, b.rkey, b.cmax, b.csum, b.pm);
        hipLaunchKernelGGL(k_lf_colmaxfin, dim3((L + 255) / 256, 1, g), dim3(256), 0, s, b.pm, L, nrch, b.cbest);
        hipLaunchKernelGGL(k_lf_select, dim3(1, 1, g), dim3(1024), 0, s, b.bval, b.bidx, b.cbest, L, hc, wc, 0.2f, 2,
                           b.mi + (size_t)p0 * L, b.mj + (size_t)p0 * L, b.mconf + (size_t)p0 * L, b.cnt + p0);
        MLG_LAUNCH_CHECK();
    }
    std::vector<int32_t> h_cnt(P);
    if (hipMemcpyAsync(h_cnt.data(), b.cnt, (size_t)P * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(counts, b.cnt, (size_t)P * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return MLG_EHIP;
    std::vector<int32_t> mp, ms;
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < h_cnt[p]; ++k) {
            mp.push_back(p);
            ms.push_back(k);
        }
    const long Mtot = (long)mp.size();
    for (long m0 = 0; m0 < Mtot; m0 += FINE_CHUNK) {
        const int M = (int)std::min<long>(FINE_CHUNK, Mtot - m0);
        if (hipMemcpyAsync(b.mp, mp.data() + m0, (size_t)M * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(b.ms, ms.data() + m0, (size_t)M * 4, hipMemcpyHostToDevice, s) != hipSuccess)
            return MLG_EHIP;
        const long items = (long)2 * M * 25 * 32 + (long)2 * M * 64;
        hipLaunchKernelGGL(k_lf_windows, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, fine, Hf, Wf, wc,
                           Hf / hc, b.frm, P, b.mi, b.mj, L, b.mp, b.ms, M, bc.x, b.win, b.crow);
        MLG_LAUNCH_CHECK();
        const long frows = (long)2 * M * 25;
        // merge_feat on [window | down_proj(coarse)]: the window half per token, the
        // coarse half once per (side, match)
        MLG_TRY(mlg_gemm_conv(b.win, 128, (const bf16_t*)w.merge_wf, nullptr, nullptr, 0, bf.t, 128, nullptr, 0, 0, 0,
                             (int)frows, 128, 128, s));
        MLG_TRY(mlg_gemm_conv(b.crow, 256, (const bf16_t*)w.down_w, w.down_b, nullptr, 0, nullptr, 0, b.cd, 128, 0, 0,
                             2 * M, 128, 256, s));
        MLG_TRY(mlg_gemm_conv(b.cd, 128, (const bf16_t*)w.merge_wc, w.merge_b, nullptr, 0, b.cm, 128, nullptr, 0, 0, 0,
                             2 * M, 128, 128, s));
        hipLaunchKernelGGL(k_lf_fine_tokens, dim3((unsigned)((frows * 32 + 255) / 256)), dim3(256), 0, s, bf.t, b.cm,
                           frows, bf.x, bf.cat);
        MLG_LAUNCH_CHECK();
        MLG_TRY(transformer(w.fine, 2, bf, 128, M, 25, s));
        hipLaunchKernelGGL(k_lf_fine_match, dim3(M), dim3(64), 0, s, bf.x, M, b.mp, b.ms, b.mi, b.mj, b.mconf, L, wc,
                           (float)H / (float)hc, (float)H / (float)Hf, kpts0, kpts1, conf);
        MLG_LAUNCH_CHECK();
        if (m0 + M < Mtot && hipStreamSynchronize(s) != hipSuccess) return MLG_EHIP;  // mp / ms reused
    }
    if (hipStreamSynchronize(s) != hipSuccess) return MLG_EHIP;  // pageable uploads complete
    return MLG_OK;
}

extern "C" size_t mlg_loftr_tails_bytes(void) { return TAILS_BYTES; }

extern "C" int mlg_set_loftr_similarity(int exact) {
    if (exact != 0 && exact != 1) return MLG_EINVAL;
    g_lf_sim_split = exact ? 0 : 1;
    return MLG_OK;
}

extern "C" int mlg_loftr_pack_tails(const mlg_loftr_weights* w, void* out, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !out) return MLG_EINVAL;
    TailW tw[8];
    return pack_tails(*w, (char*)out, tw, (hipStream_t)stream);
}

// ------------------------------------------------ op-level check of one coarse layer
namespace {
struct CoarseLayerBufs {
    LayerBufs l;  // x and cat are the caller's
    char* tails;  // room for the packed tails
};
size_t coarse_layer_carve(int nseg, int L, void* base, CoarseLayerBufs* out) {
    WsCarver c(base);
    CoarseLayerBufs b{};
    layer_carve(c, (size_t)2 * nseg * L, (size_t)2 * nseg, L, 256, true, &b.l);
    b.tails = c.take<char>(TAILS_BYTES);
    if (out) *out = b;
    return c.total();
}
}  // namespace

extern "C" size_t mlg_op_loftr_coarse_layer_ws_bytes(int nseg, int L) {
    return (nseg > 0 && L > 0) ? coarse_layer_carve(nseg, L, nullptr, nullptr) : 0;
}

// One coarse LoFTREncoderLayer `layer` (even: self on both sides; odd: cross, side 0 then
// side 1) over x f32 [2 nseg L, 256] / cat bf16 [2 nseg L, 512] (cat[:, :256] = bf16(x)),
// with the block tail fused (lg_ffn.hip, LoFTR form) or as the unfused GEMM + LayerNorm
// sequence -- the two arms of the fused-tail parity test (tests/test_loftr_gpu.py).
extern "C" int mlg_op_loftr_coarse_layer(const mlg_loftr_weights* w, int layer, int fused, float* x, uint16_t* cat,
                                         int nseg, int L, void* ws, size_t ws_bytes, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !x || !cat || !ws || layer < 0 || layer >= 8 || nseg <= 0 || L <= 0) return MLG_EINVAL;
    CoarseLayerBufs cb;
    if (coarse_layer_carve(nseg, L, ws, &cb) > ws_bytes) return MLG_ENOMEM;
    LayerBufs& b = cb.l;
    b.x = x;
    b.cat = (bf16_t*)cat;
    hipStream_t s = (hipStream_t)stream;
    TailW tails[8];
    if (fused) {
        if (w->coarse_tails)
            tails_at((char*)w->coarse_tails, tails);
        else
            MLG_TRY(pack_tails(*w, cb.tails, tails, s));
    }
    const TailW* tw = fused ? tails + layer : nullptr;
    const long half = (long)nseg * L;
    if (layer % 2 == 0) return encoder_layer(w->coarse[layer], b, 256, 0, 0, 2 * nseg, L, s, tw);
    MLG_TRY(encoder_layer(w->coarse[layer], b, 256, 0, half, nseg, L, s, tw));
    return encoder_layer(w->coarse[layer], b, 256, half, 0, nseg, L, s, tw);
}
