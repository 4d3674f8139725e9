// AnyLoc's native branch: hard-assignment VLAD over DINOv2 patch tokens, and the Lloyd
// update that fits its vocabulary (gfx950 only).
//
//   k_vlad_cnorm    c^_k = c_k / max(|c_k|, 1e-12) into a 128-row table (rows past K zero)
//   k_vlad_assign   a_i = argmax_k x_i . c^_k on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32),
//                   ties to the lowest k, and |x_i|.  x_i is not normalised first: a positive
//                   scale does not move the argmax.  The centre table is streamed through
//                   LDS in 64-channel chunks (64 x 768 f32 do not fit the LDS); every token's
//                   768 products accumulate in one fixed order, whatever its row in the tile.
//   k_vlad_agg      one workgroup per (frame, cluster), one wave per 256 channels: the frame's
//                   labels are compacted 768 at a time (ballot + prefix, stable) into a member
//                   list in LDS, and x^_i - c_k of the members is added in token order, 16 loads
//                   in flight; intra-normalises the block.
//   k_vlad_finish   the descriptor's L2 norm from the per-block sums, in cluster order.
//   k_km_changed / k_km_partial / k_km_finish   one Lloyd update: label changes, then the
//                   cluster means of x^ as per-split partial sums (token order) summed in
//                   split order.
// No floating-point atomics anywhere: a frame's descriptor does not depend on the batch.
#include "common.h"
#include "kernels.h"
#include "ws_carve.h"

namespace {

constexpr int VD = 768;          // token width
constexpr int VKMAX = 128;       // rows of the normalised centre table
constexpr int VCH = 64;          // channels per staged chunk
constexpr int VLD = VCH + 4;     // LDS row stride: 16 rows x float4 cover the 64 banks once
// k-means partial sums: at least 1536 tokens each (two gather passes), at most 256 per cluster
constexpr int KM_SPLIT_MIN = 1536, KM_SPLITS_MAX = 256;

__global__ __launch_bounds__(64) void k_vlad_cnorm(const float* __restrict__ C, int K, float* __restrict__ Chat) {
    const int k = blockIdx.x, lane = threadIdx.x;
    float* y = Chat + (size_t)k * VD;
    if (k >= K) {
#pragma unroll
        for (int j = 0; j < VD / 64; ++j) y[lane + 64 * j] = 0.f;
        return;
    }
    const float* c = C + (size_t)k * VD;
    float v[VD / 64], ss = 0.f;
#pragma unroll
    for (int j = 0; j < VD / 64; ++j) {
        v[j] = c[lane + 64 * j];
        ss = fmaf(v[j], v[j], ss);
    }
    const float n = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int j = 0; j < VD / 64; ++j) y[lane + 64 * j] = v[j] / n;
}

// 64 tokens per workgroup, 16 per wave; NT tiles of 16 centres (NT * 16 >= K).  MFMA operands:
// A = centres (lane: centre l & 15, k = l >> 4), B = tokens (lane: token l & 15, k = l >> 4);
// D: lane holds token l & 15, centres 4 (l >> 4) + r.  A lane reads 4 consecutive channels
// of its token / centre row as one float4 and feeds them to 4 MFMAs, so MFMA k-index
// l >> 4 of step j is channel 4 (l >> 4) + j of the 16-channel group: the same map on
// both operands.
template <int NT>
__global__ __launch_bounds__(256) void k_vlad_assign(const float* __restrict__ X, int M,
                                                     const float* __restrict__ Chat, int K,
                                                     int32_t* __restrict__ labels, float* __restrict__ nrm) {
    __shared__ float Cs[NT * 16][VLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int row = blockIdx.x * 64 + wave * 16 + col;
    const float* x = X + (size_t)min(row, M - 1) * VD + kq * 4;  // rows past M: a clamped copy, never stored
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;
    for (int c0 = 0; c0 < VD; c0 += VCH) {
        float4 xv[VCH / 16];
#pragma unroll
        for (int s = 0; s < VCH / 16; ++s) xv[s] = *reinterpret_cast<const float4*>(x + c0 + s * 16);
        // 16 lanes write one row's 256 contiguous bytes, rows in lane order
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int e = tid + i * 256, r = e >> 4, c4 = e & 15;
            *reinterpret_cast<float4*>(&Cs[r][c4 * 4]) =
                *reinterpret_cast<const float4*>(Chat + (size_t)r * VD + c0 + c4 * 4);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < VCH / 16; ++s) {
            const float4 t = xv[s];
            ss = fmaf(t.x, t.x, ss);
            ss = fmaf(t.y, t.y, ss);
            ss = fmaf(t.z, t.z, ss);
            ss = fmaf(t.w, t.w, ss);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float4 c = *reinterpret_cast<const float4*>(&Cs[n * 16 + col][s * 16 + kq * 4]);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.x, t.x, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.y, t.y, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.z, t.z, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.w, t.w, acc[n], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // argmax, lowest k on ties: ascending k inside the lane, then across the 4 lane groups
    float best = acc[0][0];
    int bk = 4 * kq;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = n * 16 + 4 * kq + r;
            if (k < K && acc[n][r] > best) {
                best = acc[n][r];
                bk = k;
            }
        }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (ov > best || (ov == best && ok < bk)) {
            best = ov;
            bk = ok;
        }
    }
    // |x|^2: the 4 channel-quarter sums in quarter order
    float tot = __shfl(ss, col, 64);
#pragma unroll
    for (int q = 1; q < 4; ++q) tot += __shfl(ss, col + 16 * q, 64);
    if (kq == 0 && row < M) {
        labels[row] = bk;
        nrm[row] = fmaxf(sqrtf(tot), 1e-12f);
    }
}

// sum of v over the workgroup's 3 waves: butterfly per wave, then the waves in order
__device__ __forceinline__ float block3_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + sh[2];
}

// The members of cluster k among tokens [lo, hi), visited in token order by a 192-thread
// workgroup: 768 labels at a time are compacted (ballot + prefix, stable) into an index list
// in LDS, with the members' norms beside it, then every thread walks the list 16 members at a
// time -- the 16 token loads are issued together, the accumulations follow in list order --
// so the walk is not one dependent load latency per member.  acc(t, n): the thread's 4
// channels of token x_i and |x_i|.  Returns the number of members.
constexpr int GATHER = 768;
constexpr int WALK = 16;  // member loads in flight per thread
struct GatherLds {
    int mem[GATHER];
    float nrm[GATHER];
    int wsum[12];
};

template <class Acc>
__device__ __forceinline__ int for_members(const float* __restrict__ x, const float* __restrict__ nr,
                                           const int32_t* __restrict__ lab, int lo, int hi, int k, GatherLds& sh,
                                           Acc acc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int total = 0;
    for (int base = lo; base < hi; base += GATHER) {
        // thread t looks at tokens base + 192 u + t: ascending in (u, wave, lane)
        bool f[4];
        unsigned long long m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = base + u * 192 + tid;
            f[u] = p < hi && lab[p] == k;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            m[u] = __ballot(f[u]);
            if (lane == 0) sh.wsum[u * 3 + wave] = __popcll(m[u]);
        }
        __syncthreads();
        // the list position of this wave's first member of each u: every member of the
        // earlier u, then the earlier waves of the same u
        int n = 0, pre[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int w0 = sh.wsum[u * 3], w1 = sh.wsum[u * 3 + 1], w2 = sh.wsum[u * 3 + 2];
            pre[u] = n + (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0);
            n += w0 + w1 + w2;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (f[u]) {
                const int p = base + u * 192 + tid, at = pre[u] + __popcll(m[u] & ((1ull << lane) - 1));
                sh.mem[at] = p;
                sh.nrm[at] = nr[p];
            }
        __syncthreads();
        for (int j = 0; j < n; j += WALK) {
            float4 t[WALK];
#pragma unroll
            for (int u = 0; u < WALK; ++u)  // past the end: a repeated load of the last member, not accumulated
                t[u] = *reinterpret_cast<const float4*>(x + (size_t)sh.mem[min(j + u, n - 1)] * VD);
            // keep the loads up here: the compiler otherwise sinks each into its conditional
            // accumulation below, one load latency per member again
#pragma unroll
            for (int u = 0; u < WALK; ++u) asm volatile("" : "+v"(t[u].x), "+v"(t[u].y), "+v"(t[u].z), "+v"(t[u].w));
#pragma unroll
            for (int u = 0; u < WALK; ++u)
                if (j + u < n) acc(t[u], sh.nrm[j + u]);
        }
        total += n;
        __syncthreads();  // the list and the counts are rewritten by the next pass
    }
    return total;
}

// grid (K, B), 192 threads: thread t owns channels 4 t .. 4 t + 3 of cluster k in frame b
__global__ __launch_bounds__(192) void k_vlad_agg(const float* __restrict__ X, int P, const float* __restrict__ C,
                                                  int K, const int32_t* __restrict__ labels,
                                                  const float* __restrict__ nrm, float* __restrict__ desc,
                                                  float* __restrict__ part) {
    __shared__ float sh[3];
    __shared__ GatherLds gl;
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float4 c = *reinterpret_cast<const float4*>(C + (size_t)k * VD + tid * 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for_members(X + (size_t)b * P * VD + tid * 4, nrm + (size_t)b * P, labels + (size_t)b * P, 0, P, k, gl,
                [&](const float4& t, float n) {
                    v.x += t.x / n - c.x;
                    v.y += t.y / n - c.y;
                    v.z += t.z / n - c.z;
                    v.w += t.w / n - c.w;
                });
    const float n = fmaxf(sqrtf(block3_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w, sh)), 1e-12f);
    v.x /= n;
    v.y /= n;
    v.z /= n;
    v.w /= n;
    *reinterpret_cast<float4*>(desc + ((size_t)b * K + k) * VD + tid * 4) = v;
    const float s2 = block3_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w, sh);
    if (tid == 0) part[(size_t)b * K + k] = s2;
}

__global__ __launch_bounds__(192) void k_vlad_finish(float* __restrict__ desc, const float* __restrict__ part, int K) {
    const int k = blockIdx.x, b = blockIdx.y;
    const float* pb = part + (size_t)b * K;
    float tot = 0.f;
    for (int j = 0; j < K; ++j) tot += pb[j];
    const float n = fmaxf(sqrtf(tot), 1e-12f);
    float4* d = reinterpret_cast<float4*>(desc + ((size_t)b * K + k) * VD + threadIdx.x * 4);
    float4 v = *d;
    v.x /= n;
    v.y /= n;
    v.z /= n;
    v.w /= n;
    *d = v;
}

// labels <- newl; *changed += the number of rows whose label moved (integer atomic)
__global__ __launch_bounds__(256) void k_km_changed(const int32_t* __restrict__ newl, int32_t* __restrict__ labels,
                                                    int M, unsigned long long* __restrict__ changed) {
    int c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)M; i += (size_t)gridDim.x * 256) {
        const int32_t a = newl[i];
        c += a != labels[i];
        labels[i] = a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(changed, (unsigned long long)c);
}

// grid (splits, K), 192 threads: sum of x^ over cluster k's members among tokens
// [s L, (s + 1) L), in token order, and their number
__global__ __launch_bounds__(192) void k_km_partial(const float* __restrict__ X, int M, int L,
                                                    const int32_t* __restrict__ labels,
                                                    const float* __restrict__ nrm, float* __restrict__ psum,
                                                    int32_t* __restrict__ pcnt) {
    __shared__ GatherLds gl;
    const int s = blockIdx.x, k = blockIdx.y, K = gridDim.y, tid = threadIdx.x;
    const int lo = s * L, hi = min(M, lo + L);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int cnt = for_members(X + tid * 4, nrm, labels, lo, hi, k, gl, [&](const float4& t, float n) {
        v.x += t.x / n;
        v.y += t.y / n;
        v.z += t.z / n;
        v.w += t.w / n;
    });
    *reinterpret_cast<float4*>(psum + ((size_t)s * K + k) * VD + tid * 4) = v;
    if (tid == 0) pcnt[s * K + k] = cnt;
}

// grid K, 192 threads: the partial sums in split order; an empty cluster keeps its centre
__global__ __launch_bounds__(192) void k_km_finish(const float* __restrict__ psum, const int32_t* __restrict__ pcnt,
                                                   int S, float* __restrict__ centers, int32_t* __restrict__ counts) {
    const int k = blockIdx.x, K = gridDim.x, tid = threadIdx.x;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
        const float4 t = *reinterpret_cast<const float4*>(psum + ((size_t)s * K + k) * VD + tid * 4);
        v.x += t.x;
        v.y += t.y;
        v.z += t.z;
        v.w += t.w;
        cnt += pcnt[s * K + k];
    }
    if (tid == 0) counts[k] = cnt;
    if (cnt == 0) return;
    const float n = (float)cnt;
    *reinterpret_cast<float4*>(centers + (size_t)k * VD + tid * 4) = make_float4(v.x / n, v.y / n, v.z / n, v.w / n);
}

struct VladWs {
    float *chat, *nrm, *part;
    int32_t* labels;
};

VladWs vlad_take(WsCarver& c, size_t rows, int B, int K) {
    VladWs o;
    o.chat = c.take<float>((size_t)VKMAX * VD);
    o.nrm = c.take<float>(rows);
    o.labels = c.take<int32_t>(rows);
    o.part = c.take<float>((size_t)B * K);
    return o;
}

size_t vlad_carve(size_t rows, int B, int K, void* base, VladWs* w) {
    WsCarver c(base);
    const VladWs o = vlad_take(c, rows, B, K);
    if (w) *w = o;
    return c.total();
}

int km_split_len(long M) {
    const long l = std::max<long>(KM_SPLIT_MIN, (M + KM_SPLITS_MAX - 1) / KM_SPLITS_MAX);
    return (int)((l + 63) / 64 * 64);
}

struct KmWs {
    VladWs v;
    float* psum;
    int32_t* pcnt;
};

// the VLAD head's buffers for one "frame" of M tokens, then the per-split partial sums
size_t km_carve(long M, int K, void* base, KmWs* w) {
    WsCarver c(base);
    KmWs o;
    o.v = vlad_take(c, (size_t)M, 1, K);
    const size_t S = (size_t)ceil_div(M, km_split_len(M));
    o.psum = c.take<float>(S * K * VD);
    o.pcnt = c.take<int32_t>(S * K);
    if (w) *w = o;
    return c.total();
}

bool vlad_k_ok(int K) { return K >= 16 && K <= VKMAX && K % 16 == 0; }

// labels and norms of M token rows against the centres (both validated by the caller)
int vlad_assign(const float* centers, int K, const float* tokens, int M, const VladWs& w, int32_t* labels,
                hipStream_t s) {
    hipLaunchKernelGGL(k_vlad_cnorm, dim3(VKMAX), dim3(64), 0, s, centers, K, w.chat);
    MLG_LAUNCH_CHECK();
    const dim3 grid(ceil_div(M, 64)), block(256);
    if (K <= 16)
        hipLaunchKernelGGL(k_vlad_assign<1>, grid, block, 0, s, tokens, M, w.chat, K, labels, w.nrm);
    else if (K <= 32)
        hipLaunchKernelGGL(k_vlad_assign<2>, grid, block, 0, s, tokens, M, w.chat, K, labels, w.nrm);
    else if (K <= 64)
        hipLaunchKernelGGL(k_vlad_assign<4>, grid, block, 0, s, tokens, M, w.chat, K, labels, w.nrm);
    else
        hipLaunchKernelGGL(k_vlad_assign<8>, grid, block, 0, s, tokens, M, w.chat, K, labels, w.nrm);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

constexpr long ROWS_MAX = 1L << 30;  // row indices plus a tile / gather pass / k-means split stay in int

}  // namespace

size_t mlg_vlad_ws_bytes(int B, int P, int K) {
    if (B <= 0 || P <= 0 || B > 65535 || !vlad_k_ok(K) || (long)B * P > ROWS_MAX) return 0;
    return vlad_carve((size_t)B * P, B, K, nullptr, nullptr);
}

int mlg_vlad_run(const float* centers, int K, const float* tokens, int B, int P, void* ws, size_t ws_bytes,
                 float* desc, int32_t* labels, hipStream_t s) {
    if (!mlg_vlad_ws_bytes(B, P, K) || !centers || !tokens || !ws || !desc) return MLG_EINVAL;
    if (((uintptr_t)tokens | (uintptr_t)centers | (uintptr_t)desc) & 15) return MLG_EINVAL;  // float4 access
    VladWs w;
    if (vlad_carve((size_t)B * P, B, K, ws, &w) > ws_bytes) return MLG_EINVAL;
    if (!labels) labels = w.labels;
    MLG_TRY(vlad_assign(centers, K, tokens, B * P, w, labels, s));
    hipLaunchKernelGGL(k_vlad_agg, dim3(K, B), dim3(192), 0, s, tokens, P, centers, K, labels, w.nrm, desc, w.part);
    MLG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vlad_finish, dim3(K, B), dim3(192), 0, s, desc, w.part, K);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}

size_t mlg_kmeans_ws_bytes(long M, int K) {
    if (M <= 0 || M > ROWS_MAX || !vlad_k_ok(K)) return 0;
    return km_carve(M, K, nullptr, nullptr);
}

int mlg_kmeans_step_run(const float* tokens, long M, float* centers, int K, int32_t* labels, int64_t* changed,
                        int32_t* counts, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!mlg_kmeans_ws_bytes(M, K) || !tokens || !centers || !labels || !changed || !counts || !ws) return MLG_EINVAL;
    if (((uintptr_t)tokens | (uintptr_t)centers) & 15) return MLG_EINVAL;
    KmWs w;
    if (km_carve(M, K, ws, &w) > ws_bytes) return MLG_EINVAL;
    MLG_TRY(vlad_assign(centers, K, tokens, (int)M, w.v, w.v.labels, s));
    if (hipMemsetAsync(changed, 0, sizeof(int64_t), s) != hipSuccess) return MLG_EHIP;
    hipLaunchKernelGGL(k_km_changed, dim3(std::min(1024, ceil_div(M, 256))), dim3(256), 0, s, w.v.labels, labels,
                       (int)M, reinterpret_cast<unsigned long long*>(changed));
    MLG_LAUNCH_CHECK();
    const int L = km_split_len(M), S = ceil_div(M, L);
    hipLaunchKernelGGL(k_km_partial, dim3(S, K), dim3(192), 0, s, tokens, (int)M, L, labels, w.v.nrm, w.psum, w.pcnt);
    MLG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_km_finish, dim3(K), dim3(192), 0, s, w.psum, w.pcnt, S, centers, counts);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
