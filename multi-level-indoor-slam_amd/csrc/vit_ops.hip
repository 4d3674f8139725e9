// Memory-bound DINOv2 ViT-S/B/L-14 ops around the GEMMs (gfx950): preprocessing + patch
// extraction, CLS rows, LayerNorm, and the fused final-LayerNorm + local-feature +
// GeM pooling of the CricaVPR descriptor.
#include "common.h"
#include "kernels.h"
#include "resize_cv.h"

#include <type_traits>

namespace {

// ----------------------------------------------------------- preprocessing ---
// CricaVPR._preprocess (place_recognition.py:781-803) fused with the patch-embed
// im2col: cv2.resize INTER_LINEAR on uint8 (OpenCV's fixed-point generic path,
// resize_cv.h), BGR/BGRA/gray -> RGB, float32 /255, float64
// (x - mean) / std, -> bf16 patch rows A[b*P + p, k], k = c*196 + ky*14 + kx
// (Conv2d weight order), zero for k in [588, Kpad).

struct PrepParams {
    const uint8_t* img;  // [B, H, W, C]
    int H, W, C, S, grid, P, Kpad;
    int swap_rb;         // 1: BGR(A) -> RGB (CricaVPR); 0: channels fed as stored (AnyLoc, :495-505)
    long img_stride;     // bytes between images
    bf16_t* out;         // [B*P, Kpad], or [B*P, 2 Kpad] = [hi | lo] rows when split
    int split;           // MLG_VIT_SPLIT: split-bf16 pairs
};

__global__ __launch_bounds__(256) void k_preprocess_patches(PrepParams pp, int total_chunks) {
    __shared__ float lut[3][256];
    for (int i = threadIdx.x; i < 768; i += 256) {
        const int c = i >> 8, u = i & 255;
        lut[c][u] = imagenet_norm(c, u);
    }
    __syncthreads();
    const int kchunks = pp.Kpad / 8;
    const int vend = resize_vec_end(pp.S * pp.C);
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total_chunks; idx += gridDim.x * 256) {
        const int row = idx / kchunks, kc = idx - row * kchunks;
        const int b = row / pp.P, p = row - b * pp.P;
        const int py = p / pp.grid, px = p - py * pp.grid;
        const uint8_t* src = pp.img + (size_t)b * pp.img_stride;
        float vals[8];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            float v2[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k = kc * 8 + e + u;
                float val = 0.f;
                if (k < 588) {
                    const int c = k / 196, rem = k - c * 196, ky = rem / 14, kx = rem - ky * 14;
                    const int y = py * 14 + ky, x = px * 14 + kx;
                    const int sc = pp.C == 1 ? 0 : (pp.swap_rb ? 2 - c : c);  // RGB c <- BGR(A) 2-c
                    const int q = resize_cv_sample(src, pp.H, pp.W, pp.C, pp.S, y, x, sc, vend);
                    val = lut[c][q];
                }
                v2[u] = val;
            }
            vals[e] = v2[0];
            vals[e + 1] = v2[1];
        }
        if (pp.split) {
            uint2 h0, l0, h1, l1;
            split_bf16x4(vals[0], vals[1], vals[2], vals[3], h0, l0);
            split_bf16x4(vals[4], vals[5], vals[6], vals[7], h1, l1);
            bf16_t* o = pp.out + (size_t)row * 2 * pp.Kpad + kc * 8;
            *reinterpret_cast<uint4*>(o) = make_uint4(h0.x, h0.y, h1.x, h1.y);
            *reinterpret_cast<uint4*>(o + pp.Kpad) = make_uint4(l0.x, l0.y, l1.x, l1.y);
        } else {
            *reinterpret_cast<uint4*>(pp.out + (size_t)row * pp.Kpad + kc * 8) =
                make_uint4(pack_bf16x2(vals[0], vals[1]), pack_bf16x2(vals[2], vals[3]), pack_bf16x2(vals[4], vals[5]),
                           pack_bf16x2(vals[6], vals[7]));
        }
    }
}

// X[b, 0, :] = cls + pos[0]
template <int E>
__global__ void k_cls_rows(float* X, const float* cls, const float* pos, int T) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < E; c += blockDim.x) X[(size_t)b * T * E + c] = cls[c] + pos[c];
}

// ---------------------------------------------------------------- LayerNorm ---
// torch.nn.LayerNorm(E, eps=1e-6): biased variance, one wave per token row, E = 384 (ViT-S),
// 768 (ViT-B) or 1024 (ViT-L).  A lane holds NV vectors of W floats, vector i at column
// i * 64 W + lane * W: float4 chunks of 256 columns at 768 (3) and 1024 (4); 384 is one and a
// half such chunks, so it takes float2 chunks of 128 columns (3): 64 lanes x 6 floats, every
// wave load still a whole contiguous 512 B.
template <int E>
struct LnMap {
    using Vec = float4;
    static constexpr int W = 4, NV = E / 256;
    static_assert(E % 256 == 0, "float4 mapping: E a multiple of 256");
};
template <>
struct LnMap<384> {
    using Vec = float2;
    static constexpr int W = 2, NV = 3;
};

// per-vector pieces, fixed summation order: (x + y) + (z + w)
__device__ __forceinline__ float vsum(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float vsum(const float2& v) { return v.x + v.y; }
__device__ __forceinline__ float vsqdev(const float4& v, float mean) {
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
    return (a * a + b * b) + (c * c + d * d);
}
__device__ __forceinline__ float vsqdev(const float2& v, float mean) {
    const float a = v.x - mean, b = v.y - mean;
    return a * a + b * b;
}
__device__ __forceinline__ float4 vnorm(const float4& v, float mean, float rstd, const float4& gg, const float4& bb) {
    float4 y;
    y.x = (v.x - mean) * rstd * gg.x + bb.x;
    y.y = (v.y - mean) * rstd * gg.y + bb.y;
    y.z = (v.z - mean) * rstd * gg.z + bb.z;
    y.w = (v.w - mean) * rstd * gg.w + bb.w;
    return y;
}
__device__ __forceinline__ float2 vnorm(const float2& v, float mean, float rstd, const float2& gg, const float2& bb) {
    float2 y;
    y.x = (v.x - mean) * rstd * gg.x + bb.x;
    y.y = (v.y - mean) * rstd * gg.y + bb.y;
    return y;
}
// the pooling sums of a vector's columns: mean (AnyLoc) and GeM p = 3, clamp(min=1e-6)^3
__device__ __forceinline__ void vacc_mean(float* a, const float4& y) {
    a[0] += y.x;
    a[1] += y.y;
    a[2] += y.z;
    a[3] += y.w;
}
__device__ __forceinline__ void vacc_mean(float* a, const float2& y) {
    a[0] += y.x;
    a[1] += y.y;
}
__device__ __forceinline__ void vacc_gem(float* a, const float4& y) {
    const float c0 = fmaxf(y.x, 1e-6f), c1 = fmaxf(y.y, 1e-6f);
    const float c2 = fmaxf(y.z, 1e-6f), c3 = fmaxf(y.w, 1e-6f);
    a[0] += c0 * c0 * c0;
    a[1] += c1 * c1 * c1;
    a[2] += c2 * c2 * c2;
    a[3] += c3 * c3 * c3;
}
__device__ __forceinline__ void vacc_gem(float* a, const float2& y) {
    const float c0 = fmaxf(y.x, 1e-6f), c1 = fmaxf(y.y, 1e-6f);
    a[0] += c0 * c0 * c0;
    a[1] += c1 * c1 * c1;
}
// bf16 stores of a vector: plain, and the split pair (hi at p, lo at p + lo_col)
__device__ __forceinline__ void vstore_bf16(bf16_t* p, const float4& y) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(y.x, y.y), pack_bf16x2(y.z, y.w));
}
__device__ __forceinline__ void vstore_bf16(bf16_t* p, const float2& y) {
    *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(y.x, y.y);
}
__device__ __forceinline__ void vstore_split(bf16_t* p, int lo_col, const float4& y) {
    uint2 h, l;
    split_bf16x4(y.x, y.y, y.z, y.w, h, l);
    *reinterpret_cast<uint2*>(p) = h;
    *reinterpret_cast<uint2*>(p + lo_col) = l;
}
__device__ __forceinline__ void vstore_split(bf16_t* p, int lo_col, const float2& y) {
    const uint32_t h = pack_bf16x2(y.x, y.y);
    *reinterpret_cast<uint32_t*>(p) = h;
    *reinterpret_cast<uint32_t*>(p + lo_col) =
        pack_bf16x2(y.x - __uint_as_float(h << 16), y.y - __uint_as_float(h & 0xffff0000u));
}

template <int E>
__device__ __forceinline__ void ln_row(const float* x, const float* g, const float* bt, int lane,
                                       typename LnMap<E>::Vec (&y)[LnMap<E>::NV]) {
    using Vec = typename LnMap<E>::Vec;
    constexpr int W = LnMap<E>::W, NV = LnMap<E>::NV;
    Vec v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = *reinterpret_cast<const Vec*>(x + i * 64 * W + lane * W);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += vsum(v[i]);
    const float mean = wave_sum(s) * (1.0f / (float)E);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) q += vsqdev(v[i], mean);
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / (float)E) + 1e-6f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const Vec gg = *reinterpret_cast<const Vec*>(g + i * 64 * W + lane * W);
        const Vec bb = *reinterpret_cast<const Vec*>(bt + i * 64 * W + lane * W);
        y[i] = vnorm(v[i], mean, rstd, gg, bb);
    }
}

template <int E>
__global__ __launch_bounds__(256) void k_layernorm_bf16(const float* __restrict__ X, const float* __restrict__ g,
                                                        const float* __restrict__ b, bf16_t* __restrict__ Y, int M) {
    constexpr int W = LnMap<E>::W, NV = LnMap<E>::NV;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    typename LnMap<E>::Vec y[NV];
    ln_row<E>(X + (size_t)row * E, g, b, lane, y);
#pragma unroll
    for (int i = 0; i < NV; ++i) vstore_bf16(Y + (size_t)row * E + i * 64 * W + lane * W, y[i]);
}

// LayerNorm as split-bf16 pairs: rows of 2 E, hi in columns 0..E-1, lo in E..2E-1
template <int E>
__global__ __launch_bounds__(256) void k_layernorm_split(const float* __restrict__ X, const float* __restrict__ g,
                                                         const float* __restrict__ b, bf16_t* __restrict__ Y, int M) {
    constexpr int W = LnMap<E>::W, NV = LnMap<E>::NV;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    typename LnMap<E>::Vec y[NV];
    ln_row<E>(X + (size_t)row * E, g, b, lane, y);
#pragma unroll
    for (int i = 0; i < NV; ++i) vstore_split(Y + (size_t)row * (2 * E) + i * 64 * W + lane * W, E, y[i]);
}

// Final norm + CricaVPR heads.  get_intermediate_layers strips CLS (token 0) and the
// CricaVPR code drops the first patch (token 1): tokens 2..T-1 are the local features
// [B, T-2, E] (f32, extract_local_features) and GeM pools over exactly those.
// Block (b, chunk) normalises GEM_CHUNK tokens and writes per-chunk sums of
// clamp(x, 1e-6)^3; k_gem_finish reduces the chunks in a fixed order.
constexpr int GEM_CHUNKS = 8;

template <int E>
__global__ __launch_bounds__(256) void k_final_norm_gem(const float* __restrict__ X, const float* __restrict__ g,
                                                        const float* __restrict__ bt, float* __restrict__ local,
                                                        float* __restrict__ partial, int T, int mean_pool) {
    using Vec = typename LnMap<E>::Vec;
    constexpr int W = LnMap<E>::W, NV = LnMap<E>::NV;
    __shared__ float red[4][E];
    const int b = blockIdx.x, chunk = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = T - 2, per = (L + GEM_CHUNKS - 1) / GEM_CHUNKS;
    const int t0 = chunk * per, t1 = min(L, t0 + per);
    float acc[W * NV];
#pragma unroll
    for (int i = 0; i < W * NV; ++i) acc[i] = 0.f;
    for (int t = t0 + wave; t < t1; t += 4) {
        Vec y[NV];
        ln_row<E>(X + ((size_t)b * T + 2 + t) * E, g, bt, lane, y);
        float* dst = local ? local + ((size_t)b * L + t) * E : nullptr;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (dst) *reinterpret_cast<Vec*>(dst + i * 64 * W + lane * W) = y[i];
            if (mean_pool) vacc_mean(acc + W * i, y[i]);  // AnyLoc: patch_features.mean(dim=1)
            else vacc_gem(acc + W * i, y[i]);             // CricaVPR GeM p = 3
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < W; ++j) red[wave][i * 64 * W + lane * W + j] = acc[W * i + j];
    __syncthreads();
    for (int c = threadIdx.x; c < E; c += 256)
        partial[((size_t)b * GEM_CHUNKS + chunk) * E + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

template <int E>
__global__ void k_gem_finish(const float* __restrict__ partial, float* __restrict__ desc, int L, int mean_pool) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < E; c += blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < GEM_CHUNKS; ++k) s += partial[((size_t)b * GEM_CHUNKS + k) * E + c];
        desc[(size_t)b * E + c] = mean_pool ? s / (float)L : powf(s / (float)L, 1.0f / 3.0f);
    }
}

// Run f(std::integral_constant<int, E>) for a supported width; false otherwise.
template <class F>
bool for_width(int E, F f) {
    switch (E) {
        case 384: f(std::integral_constant<int, 384>{}); return true;
        case 768: f(std::integral_constant<int, 768>{}); return true;
        case 1024: f(std::integral_constant<int, 1024>{}); return true;
        default: return false;
    }
}

}  // namespace

int mlg_preprocess_patches(const uint8_t* img, int B, int H, int W, int C, long img_stride, int S, int Kpad,
                           int swap_rb, bf16_t* out, hipStream_t s, int split) {
    if (B <= 0 || H < 1 || W < 1 || !(C == 1 || C == 3 || C == 4) || S % 14 || Kpad < 588 || Kpad % 8)
        return MLG_EINVAL;
    PrepParams pp{img, H, W, C, S, S / 14, (S / 14) * (S / 14), Kpad, swap_rb, img_stride, out, split};
    const long total = (long)B * pp.P * (Kpad / 8);
    const int blocks = (int)std::min<long>((total + 255) / 256, 256L * 16);
    hipLaunchKernelGGL(k_preprocess_patches, dim3(blocks), dim3(256), 0, s, pp, (int)total);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

int mlg_cls_rows(float* X, const float* cls, const float* pos, int B, int T, hipStream_t s, int E) {
    if (!for_width(E, [&](auto e) {
            hipLaunchKernelGGL(k_cls_rows<decltype(e)::value>, dim3(B), dim3(256), 0, s, X, cls, pos, T);
        }))
        return MLG_EINVAL;
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

int mlg_layernorm_bf16(const float* X, const float* g, const float* b, bf16_t* Y, int M, hipStream_t s, int E) {
    if (M <= 0) return MLG_EINVAL;
    if (!for_width(E, [&](auto e) {
            hipLaunchKernelGGL(k_layernorm_bf16<decltype(e)::value>, dim3((M + 3) / 4), dim3(256), 0, s, X, g, b, Y, M);
        }))
        return MLG_EINVAL;
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

int mlg_layernorm_split(const float* X, const float* g, const float* b, bf16_t* Y, int M, hipStream_t s, int E) {
    if (M <= 0) return MLG_EINVAL;
    if (!for_width(E, [&](auto e) {
            hipLaunchKernelGGL(k_layernorm_split<decltype(e)::value>, dim3((M + 3) / 4), dim3(256), 0, s, X, g, b, Y, M);
        }))
        return MLG_EINVAL;
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

int mlg_final_norm_gem(const float* X, const float* g, const float* b, float* local, float* partial, float* desc,
                       int B, int T, int mean_pool, hipStream_t s, int E) {
    if (B <= 0 || T < 3) return MLG_EINVAL;
    if (!for_width(E, [&](auto e) {
            hipLaunchKernelGGL(k_final_norm_gem<decltype(e)::value>, dim3(B, GEM_CHUNKS), dim3(256), 0, s, X, g, b,
                               local, partial, T, mean_pool);
        }))
        return MLG_EINVAL;
    MLG_LAUNCH_CHECK();
    for_width(E, [&](auto e) {
        hipLaunchKernelGGL(k_gem_finish<decltype(e)::value>, dim3(B), dim3(256), 0, s, partial, desc, T - 2, mean_pool);
    });
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

size_t mlg_gem_partial_bytes(int B, int E) { return (size_t)B * GEM_CHUNKS * E * sizeof(float); }
