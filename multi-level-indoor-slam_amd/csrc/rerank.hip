// Re-ranking the kNN candidates by local cross-correlation inside the gate (gfx950).
//
// CricaVPR.rerank_candidates (place_recognition.py:714-757) for every query row of
// mlg_knn_gate's output, on the device and without a host synchronisation:
//
//   mlg_row_normalize_wave  every local-feature row of the bank, x / (||x|| + 1e-8), into the
//                     workspace (knn.hip: one wave per row, the bits of k_row_normalize).
//   k_rerank_xcorr    one workgroup per candidate slot (query row i, slot s); a slot that is
//                     not scored (past count, outside the mask, a frame that is not cached or
//                     out of range) leaves NaN and exits.  A live workgroup walks all
//                     128 x 128 tiles of C = qn mn^T of its pair on the exact-f32 MFMA, in
//                     sim_tile's k order (knn.hip), so every element of C has the bits
//                     k_xcorr_tiles gives it.  The row maxima of a 128-row strip stay in
//                     registers across the strip's column tiles, the L column maxima stay in
//                     LDS across the strips, and the 32 x 32 sub-blocks that lie wholly past L
//                     are skipped (a maximum does not depend on the order it is taken in, and
//                     those elements belong to neither maximum).  It ends
//                     with k_xcorr_finish's thread-strided sums, tree and root: the score is
//                     bit-identical to mlg_xcorr_batch's for the pair, in either order.
//   k_rerank_select   one wave per query row, a lane per slot (hence k <= 64): combined =
//                     0.5 float64(sim) + 0.5 float64(cross), or the global similarity alone
//                     for a candidate that was not scored; the stable descending rank of an
//                     entry is (entries with a larger score) + (earlier entries with an equal
//                     score); entries of rank < top_k are written compacted in rank order.
//                     A query frame that is not cached keeps its first top_k candidates.
#include <limits.h>

#include "common.h"
#include "kernels.h"
#include "ws_carve.h"

namespace {

constexpr int RBM = 128, RBN = 128, RBK = 16;  // sim_tile's tile (knn.hip SBM / SBN / SBK)
constexpr int RR_KMAX = 64;                    // a lane per slot
constexpr int RR_LMAX = 4096;                  // row + column maxima in LDS: 2 x 4 x L bytes

// is slot (i, s) a candidate of its row, and is it scored?  (one rule for both kernels)
struct Slot {
    bool cand, scored, qcached;
    int j;
};
__device__ __forceinline__ Slot slot_of(int i, int s, int F, int q0, int k, const int32_t* __restrict__ idx,
                                        const uint8_t* __restrict__ mask, const int32_t* __restrict__ count,
                                        const uint8_t* __restrict__ cached) {
    Slot r;
    const int cnt = min(max(count[i], 0), k);
    r.cand = s < cnt && (!mask || mask[(size_t)i * k + s] != 0);
    r.qcached = !cached || cached[q0 + i] != 0;
    r.j = s < k ? idx[(size_t)i * k + s] : -1;
    const bool in = r.j >= 0 && r.j < F;  // an index outside the bank is never read
    r.scored = r.cand && r.qcached && in && (!cached || cached[in ? r.j : 0] != 0);
    return r;
}

// One 128 x 128 tile (m0, n0) of A . B^T in sim_tile's staging and k order (knn.hip), for a
// wave whose first NA 32-row and NB 32-column sub-blocks hold an index below L: the others
// are never multiplied and take no part in the maxima.  NA / NB are template arguments so
// that the k loop has no branch between its MFMAs.  Rows / columns past L inside a live
// sub-block are clamped copies of row / column L - 1, so they repeat values the maxima
// already hold and need no mask: a maximum over duplicates is the maximum.  D % 4 == 0, so a
// float4 of k lies wholly inside D or is zero.  The next k slab's global loads are issued
// before this slab's MFMAs and land in LDS after them: the order of the products within an
// element's chain does not change.  One slab ahead, not two: the second slab's 16 registers
// cost the third wave per SIMD and the kernel ran 22 % slower.
// Folds the tile into rmx (this lane's column's share of each of the wave's rows' maxima)
// and cm (per column sub-block, the maximum over this lane's rows).
template <int NA, int NB>
__device__ __forceinline__ void rr_tile(const float* __restrict__ A, const float* __restrict__ B, int L, int D,
                                        int m0, int n0, float (&As)[RBK][RBM + 4], float (&Bs)[RBK][RBN + 4],
                                        float (&rmx)[2][16], float (&cm)[2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc[NA > 0 ? NA : 1][NB > 0 ? NB : 1];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const float* pa[2];
    const float* pb[2];
    int row[2], kq[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + i * 256;
        row[i] = e >> 2;
        kq[i] = (e & 3) * 4;
        pa[i] = A + (size_t)min(m0 + row[i], L - 1) * D + kq[i];
        pb[i] = B + (size_t)min(n0 + row[i], L - 1) * D + kq[i];
    }
    // a float4 of k past D reads the row's last float4 instead (a valid address) and is zeroed
    auto slab = [&](const float* p, int kx) {
        const bool in = kx < D;
        const float4 v = *reinterpret_cast<const float4*>(p + (in ? kx : D - 4));
        return make_float4(in ? v.x : 0.f, in ? v.y : 0.f, in ? v.z : 0.f, in ? v.w : 0.f);
    };
    float4 va[2], vb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        va[i] = slab(pa[i] - kq[i], kq[i]);
        vb[i] = slab(pb[i] - kq[i], kq[i]);
    }
    for (int k0 = 0; k0 < D; k0 += RBK) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            As[kq[i] + 0][row[i]] = va[i].x; As[kq[i] + 1][row[i]] = va[i].y;
            As[kq[i] + 2][row[i]] = va[i].z; As[kq[i] + 3][row[i]] = va[i].w;
            Bs[kq[i] + 0][row[i]] = vb[i].x; Bs[kq[i] + 1][row[i]] = vb[i].y;
            Bs[kq[i] + 2][row[i]] = vb[i].z; Bs[kq[i] + 3][row[i]] = vb[i].w;
        }
        __syncthreads();
        if (k0 + RBK < D) {  // the next slab, in flight under the MFMAs
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                va[i] = slab(pa[i] - kq[i], k0 + RBK + kq[i]);
                vb[i] = slab(pb[i] - kq[i], k0 + RBK + kq[i]);
            }
        }
        if (NA > 0 && NB > 0) {
#pragma unroll
            for (int kk = 0; kk < RBK; kk += 2) {
                const int kx = kk + (lane >> 5);
                float a[2], b[2];
#pragma unroll
                for (int t = 0; t < NA; ++t) a[t] = As[kx][wm * 64 + t * 32 + (lane & 31)];
#pragma unroll
                for (int t = 0; t < NB; ++t) b[t] = Bs[kx][wn * 64 + t * 32 + (lane & 31)];
#pragma unroll
                for (int ta = 0; ta < NA; ++ta)
#pragma unroll
                    for (int tb = 0; tb < NB; ++tb)
                        acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D[i][j]: col j = lane & 31, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int ta = 0; ta < NA; ++ta)
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int tb = 0; tb < NB; ++tb) {
                const float v = acc[ta][tb][r];
                rmx[ta][r] = fmaxf(rmx[ta][r], v);
                cm[tb] = fmaxf(cm[tb], v);
            }
}

// fn: normalised rows, frame f at fn + f * L * D.  Dynamic LDS: rowmax [Lp] | colmax [Lp],
// Lp = L rounded up to 128.
__global__ __launch_bounds__(256, 2) void k_rerank_xcorr(const float* __restrict__ fn, int F, int L, int D, int q0,
                                                         int k, const int32_t* __restrict__ idx,
                                                         const uint8_t* __restrict__ mask,
                                                         const int32_t* __restrict__ count,
                                                         const uint8_t* __restrict__ cached,
                                                         float* __restrict__ cross) {
    extern __shared__ float maxima[];
    __shared__ float As[RBK][RBM + 4];
    __shared__ float Bs[RBK][RBN + 4];
    __shared__ float part[2][2][RBM];  // [row / col][wave half][index in tile]
    __shared__ float red[2][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const unsigned slot_id = blockIdx.x;
    const int qi = (int)(slot_id / (unsigned)k), slot = (int)(slot_id % (unsigned)k);
    const Slot sl = slot_of(qi, slot, F, q0, k, idx, mask, count, cached);
    if (!sl.scored) {  // block-uniform
        if (tid == 0) cross[slot_id] = __builtin_nanf("");
        return;
    }
    const int Lp = (L + RBM - 1) / RBM * RBM;
    float* rowmax = maxima;
    float* colmax = maxima + Lp;
    for (int j = tid; j < Lp; j += 256) colmax[j] = -INFINITY;
    const float* A = fn + (size_t)(q0 + qi) * L * D;
    const float* B = fn + (size_t)sl.j * L * D;
    const int hh = lane >> 5, c = lane & 31;
    for (int m0 = 0; m0 < L; m0 += RBM) {
        // 32-row sub-blocks of this wave that hold a row below L (wave-uniform)
        const bool la[2] = {m0 + wm * 64 < L, m0 + wm * 64 + 32 < L};
        float rmx[2][16];  // this lane's column's share of each row's maximum over the strip
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int r = 0; r < 16; ++r) rmx[ta][r] = -INFINITY;
        for (int n0 = 0; n0 < L; n0 += RBN) {
            const bool lb[2] = {n0 + wn * 64 < L, n0 + wn * 64 + 32 < L};
            float cm[2] = {-INFINITY, -INFINITY};  // column max per tb over this wave's 64 rows
            // the wave's live sub-blocks (wave-uniform): one instantiation per count
            const int na = (int)la[0] + (int)la[1], nb = (int)lb[0] + (int)lb[1];
            if (na == 2 && nb == 2) rr_tile<2, 2>(A, B, L, D, m0, n0, As, Bs, rmx, cm);
            else if (na == 2 && nb == 1) rr_tile<2, 1>(A, B, L, D, m0, n0, As, Bs, rmx, cm);
            else if (na == 1 && nb == 2) rr_tile<1, 2>(A, B, L, D, m0, n0, As, Bs, rmx, cm);
            else if (na == 1 && nb == 1) rr_tile<1, 1>(A, B, L, D, m0, n0, As, Bs, rmx, cm);
            else rr_tile<0, 0>(A, B, L, D, m0, n0, As, Bs, rmx, cm);  // staging and barriers only
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) {
                const float v = fmaxf(cm[tb], __shfl_xor(cm[tb], 32, 64));  // both row halves
                if (hh == 0) part[1][wm][wn * 64 + tb * 32 + c] = v;
            }
            __syncthreads();
            if (tid < RBN && n0 + tid < L)
                colmax[n0 + tid] = fmaxf(colmax[n0 + tid], fmaxf(part[1][0][tid], part[1][1][tid]));
            // the next write of part[1] comes after the next tile's k loop (two barriers)
        }
        // the strip's row maxima: across the 32 lanes of a half (columns), then both halves
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float rm = rmx[ta][r];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) rm = fmaxf(rm, __shfl_xor(rm, o, 64));
                if (c == 0) part[0][wn][wm * 64 + ta * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh] = rm;
            }
        __syncthreads();
        if (tid < RBM && m0 + tid < L) rowmax[m0 + tid] = fmaxf(part[0][0][tid], part[0][1][tid]);
    }
    __syncthreads();
    // k_xcorr_finish's sums, tree and root
    float rs = 0.f, cs = 0.f;
    for (int i = tid; i < L; i += 256) rs += rowmax[i];
    for (int j = tid; j < L; j += 256) cs += colmax[j];
    red[0][tid] = rs;
    red[1][tid] = cs;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) cross[slot_id] = sqrtf((red[0][0] / (float)L) * (red[1][0] / (float)L));
}

__global__ __launch_bounds__(64) void k_rerank_select(int F, int q0, int k, int top_k, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ sim,
                                                      const uint8_t* __restrict__ mask,
                                                      const int32_t* __restrict__ count,
                                                      const uint8_t* __restrict__ cached,
                                                      const float* __restrict__ cross, int32_t* __restrict__ r_idx,
                                                      float* __restrict__ r_sim, float* __restrict__ r_cross,
                                                      double* __restrict__ r_score, int32_t* __restrict__ r_count,
                                                      unsigned long long* __restrict__ dropped) {
    const int i = blockIdx.x, s = threadIdx.x;
    const Slot sl = slot_of(i, s, F, q0, k, idx, mask, count, cached);
    const float g = s < k ? sim[(size_t)i * k + s] : 0.f;
    const float cr = sl.scored ? cross[(size_t)i * k + s] : __builtin_nanf("");
    const double sc = sl.scored ? 0.5 * (double)g + 0.5 * (double)cr : (double)g;
    const unsigned long long cands = __ballot(sl.cand);
    int rank;
    if (sl.qcached) {  // wave-uniform
        rank = 0;
        for (int t = 0; t < k; ++t) {
            const double st = __shfl(sc, t, 64);
            if (((cands >> t) & 1) && (st > sc || (st == sc && t < s))) ++rank;
        }
    } else {
        rank = __popcll(cands & ((1ull << s) - 1));  // the first top_k candidates, unchanged
    }
    const int ncand = __popcll(cands), kept = min(ncand, top_k);
    const size_t o = (size_t)i * top_k;
    if (sl.cand && rank < top_k) {
        r_idx[o + rank] = sl.j;
        r_sim[o + rank] = g;
        r_cross[o + rank] = cr;
        r_score[o + rank] = sc;
    }
    if (s >= kept && s < top_k) {  // past the kept entries: a fixed filler
        r_idx[o + s] = -1;
        r_sim[o + s] = 0.f;
        r_cross[o + s] = __builtin_nanf("");
        r_score[o + s] = 0.0;
    }
    if (s == 0) {
        r_count[i] = kept;
        if (dropped && ncand > kept) atomicAdd(dropped, (unsigned long long)(ncand - kept));
    }
}

struct RrBufs {
    float *fn, *cross;  // normalised rows [F, L, D]; cross score per slot [Q, k] (NaN: not scored)
};

bool rr_shape_ok(int F, int L, int D, int Q, int k) {
    return F > 0 && L > 0 && D > 0 && Q > 0 && k >= 1 && k <= RR_KMAX && D % 4 == 0 && L <= RR_LMAX
           && (long long)F * L <= INT_MAX && (long long)Q * k <= INT_MAX;
}

size_t rr_carve(int F, int L, int D, int Q, int k, void* base, RrBufs* out) {
    WsCarver c(base);
    RrBufs b;
    b.fn = c.take<float>((size_t)F * L * D);
    b.cross = c.take<float>((size_t)Q * k);
    if (out) *out = b;
    return c.total();
}

}  // namespace

size_t mlg_rerank_ws_bytes(int F, int L, int D, int Q, int k) {
    if (!rr_shape_ok(F, L, D, Q, k)) return 0;
    return rr_carve(F, L, D, Q, k, nullptr, nullptr);
}

int mlg_rerank_run(const float* feats, int F, int L, int D, int q0, int Q, int k, const int32_t* idx,
                   const float* sim, const uint8_t* mask, const int32_t* count, const uint8_t* cached, int top_k,
                   void* ws, size_t ws_bytes, int32_t* r_idx, float* r_sim, float* r_cross, double* r_score,
                   int32_t* r_count, unsigned long long* dropped, hipStream_t s) {
    if (!feats || !idx || !sim || !count || !ws || !r_idx || !r_sim || !r_cross || !r_score || !r_count)
        return MLG_EINVAL;
    if (!rr_shape_ok(F, L, D, Q, k) || top_k < 1 || top_k > k || q0 < 0 || (long long)q0 + Q > F) return MLG_EINVAL;
    RrBufs b;
    if (rr_carve(F, L, D, Q, k, ws, &b) > ws_bytes) return MLG_ENOMEM;
    // the reference's q / (||q|| + 1e-8) per row, numpy-exact, one wave per row
    MLG_TRY(mlg_row_normalize_wave(feats, b.fn, F * L, D, nullptr, s));
    const int Lp = (L + RBM - 1) / RBM * RBM;
    hipLaunchKernelGGL(k_rerank_xcorr, dim3((unsigned)Q * (unsigned)k), dim3(256), 2 * Lp * sizeof(float), s, b.fn, F,
                       L, D, q0, k, idx, mask, count, cached, b.cross);
    hipLaunchKernelGGL(k_rerank_select, dim3(Q), dim3(64), 0, s, F, q0, k, top_k, idx, sim, mask, count, cached,
                       b.cross, r_idx, r_sim, r_cross, r_score, r_count, dropped);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
