// CricaVPR's native branch (include/mlgate.h "CricaVPR head"): the 14-region GeM pyramid over
// the final-normed DINOv2 tokens and the 2-layer cross-image transformer encoder, f32
// element-wise work around the split-bf16 GEMM launchers of gemm_bf16.hip.
//
//   k_crica_pool       final LayerNorm of CLS + g^2 patch tokens, per-token L2 normalisation,
//                      clamp, x^p, the 4 + 9 region sums in token order, ^(1/p)
//   k_crica_rows       a row pass over [14 B, 768]: optional LayerNorm (eps 1e-5) in place,
//                      and the [hi | lo] bf16 operand of the next GEMM
//   k_crica_attention  per (group, region, head): G x G scores over 48 dims, softmax, P V
//   k_crica_finish     the 10752-wide L2 normalisation, one frame per workgroup
//
// Every sum has a fixed order that depends only on the frame's own group: no floating-point
// atomics, no scratch; a GEMM row depends on no other row.  So a group's descriptors are the
// same bits wherever the group sits in a call.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "ws_carve.h"

namespace {

constexpr int E = MLG_VIT_EMBED, ROWS = MLG_CRICA_ROWS, HEADS = 16, HD = 48, FF = 2048;
constexpr int MAX_GRID = 64;  // k_crica_pool keeps 3 floats per patch token in LDS: 48 KiB at 64 x 64

// one 768-wide row held by a wave as 3 float4 per lane: two-pass LayerNorm statistics
__device__ __forceinline__ void row_load(const float* x, int lane, float4 v[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = *reinterpret_cast<const float4*>(x + i * 256 + lane * 4);
}

__device__ __forceinline__ void row_stats(const float4 v[3], float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    mean = wave_sum(s) * (1.0f / E);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        q += (a * a + b * b) + (c * c + d * d);
    }
    rstd = rsqrtf(wave_sum(q) * (1.0f / E) + eps);
}

__device__ __forceinline__ void row_affine(const float4 v[3], float mean, float rstd, const float* __restrict__ g,
                                           const float* __restrict__ bt, int lane, float4 y[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 gg = *reinterpret_cast<const float4*>(g + i * 256 + lane * 4);
        const float4 bb = *reinterpret_cast<const float4*>(bt + i * 256 + lane * 4);
        y[i].x = (v[i].x - mean) * rstd * gg.x + bb.x;
        y[i].y = (v[i].y - mean) * rstd * gg.y + bb.y;
        y[i].z = (v[i].z - mean) * rstd * gg.z + bb.z;
        y[i].w = (v[i].w - mean) * rstd * gg.w + bb.w;
    }
}

// Pyramid GeM of one frame per workgroup of 768 threads.  Phase 1, a wave per token: the
// final LayerNorm (eps 1e-6), the CLS row out, and per patch token (mean, rstd, the L2 norm of
// its normed row) into LDS.  Phase 2, a thread per channel: the tokens in
// row-major order, each added into its level-1 and its level-2 region; a band of regions is
// finished (mean, ^(1/p)) when its last patch row has passed.  The column cuts 5, 8, 11 split
// a patch row into four runs with fixed (level-1, level-2) column bands.  The residual stream
// is read from memory once per phase; the second read is served by the caches.
__global__ __launch_bounds__(768) void k_crica_pool(const float* __restrict__ X, const float* __restrict__ g,
                                                    const float* __restrict__ bt, int grid, float p,
                                                    float* __restrict__ out) {
    extern __shared__ float stats[];  // [P][3]: mean, rstd, max(|y|, 1e-12)
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = grid * grid;
    const float* xb = X + (size_t)b * (P + 1) * E;
    float* ob = out + (size_t)b * ROWS * E;
    for (int t = wave; t <= P; t += 12) {
        float4 v[3], y[3];
        float mean, rstd;
        row_load(xb + (size_t)t * E, lane, v);
        row_stats(v, 1e-6f, mean, rstd);
        row_affine(v, mean, rstd, g, bt, lane, y);
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) *reinterpret_cast<float4*>(ob + i * 256 + lane * 4) = y[i];
            continue;
        }
        float n2 = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) n2 += (y[i].x * y[i].x + y[i].y * y[i].y) + (y[i].z * y[i].z + y[i].w * y[i].w);
        const float nrm = fmaxf(sqrtf(wave_sum(n2)), 1e-12f);
        if (lane == 0) {
            stats[3 * (t - 1) + 0] = mean;
            stats[3 * (t - 1) + 1] = rstd;
            stats[3 * (t - 1) + 2] = nrm;
        }
    }
    __syncthreads();

    const int c = tid;
    const float gc = g[c], bc = bt[c], ip = 1.0f / p;
    auto term = [&](int t) {
        const float* st = stats + 3 * t;
        const float y = (xb[(size_t)(t + 1) * E + c] - st[0]) * st[1] * gc + bc;
        return powf(fmaxf(y / st[2], 1e-6f), p);
    };
    float a1[2] = {0.f, 0.f}, a2[3] = {0.f, 0.f, 0.f};
    for (int r = 0; r < grid; ++r) {
        const int t0 = r * grid;
        for (int col = 0; col < 5; ++col) {
            const float w = term(t0 + col);
            a1[0] += w;
            a2[0] += w;
        }
        for (int col = 5; col < 8; ++col) {
            const float w = term(t0 + col);
            a1[0] += w;
            a2[1] += w;
        }
        for (int col = 8; col < 11; ++col) {
            const float w = term(t0 + col);
            a1[1] += w;
            a2[1] += w;
        }
        for (int col = 11; col < grid; ++col) {
            const float w = term(t0 + col);
            a1[1] += w;
            a2[2] += w;
        }
        if (r == 7 || r == grid - 1) {  // level 1: patch rows [0:8], [8:g] x columns [0:8], [8:g]
            const int band = r == 7 ? 0 : 1, nr = r == 7 ? 8 : grid - 8;
            ob[(size_t)(1 + band * 2 + 0) * E + c] = powf(a1[0] / (float)(nr * 8), ip);
            ob[(size_t)(1 + band * 2 + 1) * E + c] = powf(a1[1] / (float)(nr * (grid - 8)), ip);
            a1[0] = a1[1] = 0.f;
        }
        if (r == 4 || r == 10 || r == grid - 1) {  // level 2: [0:5], [5:11], [11:g] both ways
            const int band = r == 4 ? 0 : r == 10 ? 1 : 2, nr = r == 4 ? 5 : r == 10 ? 6 : grid - 11;
            ob[(size_t)(5 + band * 3 + 0) * E + c] = powf(a2[0] / (float)(nr * 5), ip);
            ob[(size_t)(5 + band * 3 + 1) * E + c] = powf(a2[1] / (float)(nr * 6), ip);
            ob[(size_t)(5 + band * 3 + 2) * E + c] = powf(a2[2] / (float)(nr * (grid - 11)), ip);
            a2[0] = a2[1] = a2[2] = 0.f;
        }
    }
}

// A wave per row of [M, 768].  NORM: x = LayerNorm(x) (eps 1e-5, nn.TransformerEncoderLayer's)
// written back to X; else X = src.  Both write the row's split operand [hi | lo] to XS.
template <bool NORM>
__global__ __launch_bounds__(256) void k_crica_rows(const float* src, float* X,  // NORM: src == X
                                                    const float* __restrict__ g, const float* __restrict__ bt,
                                                    bf16_t* __restrict__ XS, int M) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float4 v[3], y[3];
    row_load(src + (size_t)row * E, lane, v);
    if (NORM) {
        float mean, rstd;
        row_stats(v, 1e-5f, mean, rstd);
        row_affine(v, mean, rstd, g, bt, lane, y);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) y[i] = v[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        uint2 h, l;
        split_bf16x4(y[i].x, y[i].y, y[i].z, y[i].w, h, l);
        *reinterpret_cast<float4*>(X + (size_t)row * E + i * 256 + lane * 4) = y[i];
        *reinterpret_cast<uint2*>(XS + (size_t)row * 2 * E + i * 256 + lane * 4) = h;
        *reinterpret_cast<uint2*>(XS + (size_t)row * 2 * E + E + i * 256 + lane * 4) = l;
    }
}

// nn.MultiheadAttention over the image axis: frames [j G, min((j + 1) G, B)) are group j, and
// row r of a frame attends over row r of the frames of its group.  QKV f32 [14 B, 2304] =
// [q | k | v], 16 heads of 48.  A workgroup is (group, region, 4 heads); 32 lanes per head,
// lane i the query of the group's frame i.  K and V of the head sit in LDS and are read as
// broadcasts; scores, softmax and P V are sequential f32 sums in key order.  O: the split operand
// [hi | lo] of out_proj, [14 B, 2 x 768].
__global__ __launch_bounds__(128) void k_crica_attention(const float* __restrict__ QKV, bf16_t* __restrict__ O, int B,
                                                         int G) {
    __shared__ __attribute__((aligned(16))) float Ks[4][32][HD];
    __shared__ __attribute__((aligned(16))) float Vs[4][32][HD];
    const int r = blockIdx.y, hq = threadIdx.x >> 5, h = blockIdx.z * 4 + hq, i = threadIdx.x & 31;
    const int f0 = blockIdx.x * G, n = min(G, B - f0);
    for (int e = i; e < n * (HD / 4); e += 32) {
        const int kk = e / (HD / 4), d = (e % (HD / 4)) * 4;
        const float* src = QKV + ((size_t)(f0 + kk) * ROWS + r) * (3 * E) + h * HD + d;
        *reinterpret_cast<float4*>(&Ks[hq][kk][d]) = *reinterpret_cast<const float4*>(src + E);
        *reinterpret_cast<float4*>(&Vs[hq][kk][d]) = *reinterpret_cast<const float4*>(src + 2 * E);
    }
    __syncthreads();
    if (i >= n) return;
    const size_t row = (size_t)(f0 + i) * ROWS + r;
    float q[HD];
    const float scale = 0.14433756729740643f;  // 48^-1/2
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        const float4 t = *reinterpret_cast<const float4*>(QKV + row * (3 * E) + h * HD + d);
        q[d] = t.x * scale;
        q[d + 1] = t.y * scale;
        q[d + 2] = t.z * scale;
        q[d + 3] = t.w * scale;
    }
    // two passes in key order: the row maximum, then e_k = exp(s_k - max) with the scores
    // computed again (48 FMAs; no per-lane score array), sum e_k and sum e_k V_k; out = the
    // latter over the former
    auto score = [&](int kk) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) s = fmaf(q[d], Ks[hq][kk][d], s);
        return s;
    };
    float m = -INFINITY;
#pragma unroll 1
    for (int kk = 0; kk < n; ++kk) m = fmaxf(m, score(kk));
    float sum = 0.f, acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll 1
    for (int kk = 0; kk < n; ++kk) {
        const float e = expf(score(kk) - m);
        sum += e;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc[d] = fmaf(e, Vs[hq][kk][d], acc[d]);
    }
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] /= sum;
    bf16_t* dst = O + row * (2 * E) + h * HD;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        uint2 hi, lo;
        split_bf16x4(acc[d], acc[d + 1], acc[d + 2], acc[d + 3], hi, lo);
        *reinterpret_cast<uint2*>(dst + d) = hi;
        *reinterpret_cast<uint2*>(dst + E + d) = lo;
    }
}

// desc[b] = x[b] / max(|x[b]|, 1e-12) over the frame's 14 x 768 values: per-thread strided
// sums, a wave reduction, the four waves' sums in wave order
__global__ __launch_bounds__(256) void k_crica_finish(const float* __restrict__ X, float* __restrict__ desc) {
    __shared__ float part[4];
    const float* x = X + (size_t)blockIdx.x * MLG_CRICA_DIM;
    float* d = desc + (size_t)blockIdx.x * MLG_CRICA_DIM;
    float s = 0.f;
    for (int k = threadIdx.x; k < MLG_CRICA_DIM; k += 256) s = fmaf(x[k], x[k], s);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    const float nrm = fmaxf(sqrtf((part[0] + part[1]) + (part[2] + part[3])), 1e-12f);
    for (int k = threadIdx.x; k < MLG_CRICA_DIM; k += 256) d[k] = x[k] / nrm;
}

__global__ void k_crica_fill(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

struct CricaBufs {
    float *x, *qkv, *ones;  // [M, 768] the stream; [M, 2304] in_proj's output; 2304 ones (the launchers' gamma)
    bf16_t *xs, *o, *h;     // split operands: [M, 2 x 768] x2, [M, 2 x 2048]
};

size_t crica_carve(int B, void* base, CricaBufs* out) {
    const size_t M = (size_t)B * ROWS;
    WsCarver c(base);
    CricaBufs b;
    b.x = c.take<float>(M * E);
    b.xs = c.take<bf16_t>(M * 2 * E);
    b.qkv = c.take<float>(M * 3 * E);
    b.o = c.take<bf16_t>(M * 2 * E);
    b.h = c.take<bf16_t>(M * 2 * FF);
    b.ones = c.take<float>(3 * E);
    if (out) *out = b;
    return c.total();
}

bool aligned16(const void* p) { return p && !(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

bool mlg_crica_weights_ok(const mlg_crica_weights& cw) {
    if (!(cw.gem_p > 0.f) || !isfinite(cw.gem_p)) return false;
    for (const mlg_crica_layer& l : cw.layers) {
        const void* ptrs[] = {l.in_w, l.in_b, l.out_w, l.out_b, l.ln1_g, l.ln1_b,
                              l.fc1_w, l.fc1_b, l.fc2_w, l.fc2_b, l.ln2_g, l.ln2_b};
        for (const void* p : ptrs)
            if (!aligned16(p)) return false;
    }
    return true;
}

size_t mlg_crica_head_ws_bytes(int B) {
    if (B < 1 || B > MLG_CRICA_MAX_BATCH) return 0;
    return crica_carve(B, nullptr, nullptr);
}

int mlg_crica_pool_run(const float* tokens, const float* norm_w, const float* norm_b, int B, int grid, float gem_p,
                       float* out, hipStream_t s) {
    if (!aligned16(tokens) || !aligned16(norm_w) || !aligned16(norm_b) || !aligned16(out)) return MLG_EINVAL;
    if (B < 1 || B > MLG_CRICA_MAX_BATCH || grid < MLG_CRICA_MIN_GRID || grid > MAX_GRID) return MLG_EINVAL;
    if (!(gem_p > 0.f) || !isfinite(gem_p)) return MLG_EINVAL;
    hipLaunchKernelGGL(k_crica_pool, dim3(B), dim3(768), (size_t)grid * grid * 3 * sizeof(float), s, tokens, norm_w,
                       norm_b, grid, gem_p, out);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

int mlg_crica_encoder_run(const mlg_crica_weights& cw, const float* pooled, int B, int group, void* ws,
                          size_t ws_bytes, float* desc, hipStream_t s) {
    if (!mlg_crica_weights_ok(cw) || !aligned16(pooled) || !aligned16(ws) || !aligned16(desc)) return MLG_EINVAL;
    if (B < 1 || B > MLG_CRICA_MAX_BATCH || group < 1 || group > MLG_CRICA_MAX_GROUP) return MLG_EINVAL;
    CricaBufs b;
    if (crica_carve(B, ws, &b) > ws_bytes) return MLG_ENOMEM;
    const int M = B * ROWS, rowblocks = (M + 3) / 4, ngroups = (B + group - 1) / group;
    hipLaunchKernelGGL(k_crica_fill, dim3((3 * E + 255) / 256), dim3(256), 0, s, b.ones, 3 * E, 1.0f);
    MLG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_crica_rows<false>, dim3(rowblocks), dim3(256), 0, s, pooled, b.x, nullptr, nullptr, b.xs, M);
    MLG_LAUNCH_CHECK();
    for (const mlg_crica_layer& l : cw.layers) {
        // an f32 GEMM output is the residual launcher on a zeroed target with gamma = 1
        if (hipMemsetAsync(b.qkv, 0, (size_t)M * 3 * E * sizeof(float), s) != hipSuccess) return MLG_EHIP;
        MLG_TRY(mlg_gemm_residual_split(b.xs, l.in_w, l.in_b, b.ones, b.qkv, M, 3 * E, E, s));
        hipLaunchKernelGGL(k_crica_attention, dim3(ngroups, ROWS, HEADS / 4), dim3(128), 0, s, b.qkv, b.o, B, group);
        MLG_LAUNCH_CHECK();
        // post-LN: x = LN1(x + out_proj(attention)); the add is the launcher's residual
        MLG_TRY(mlg_gemm_residual_split(b.o, l.out_w, l.out_b, b.ones, b.x, M, E, E, s));
        hipLaunchKernelGGL(k_crica_rows<true>, dim3(rowblocks), dim3(256), 0, s, b.x, b.x, l.ln1_g, l.ln1_b, b.xs, M);
        MLG_LAUNCH_CHECK();
        // x = LN2(x + fc2(gelu(fc1(x))))
        MLG_TRY(mlg_gemm_bias_gelu_split(b.xs, l.fc1_w, l.fc1_b, b.h, M, FF, E, s));
        MLG_TRY(mlg_gemm_residual_split(b.h, l.fc2_w, l.fc2_b, b.ones, b.x, M, E, FF, s));
        hipLaunchKernelGGL(k_crica_rows<true>, dim3(rowblocks), dim3(256), 0, s, b.x, b.x, l.ln2_g, l.ln2_b, b.xs, M);
        MLG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_crica_finish, dim3(B), dim3(256), 0, s, b.x, desc);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
