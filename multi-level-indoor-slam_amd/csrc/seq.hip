// Sequence-consistency check of the kNN candidates inside the gate (gfx950).
//
// The rule is stated once, in include/mlgate.h (mlg_seq_gate).  In short: a candidate
// (i, j) of mlg_knn_gate's lists is scored by the mean similarity of the frames i + d and
// j + dir d over d in [-w, w], in both travel directions, and kept when the better
// direction's mean reaches the threshold.
//
//   mlg_row_normalize_wave  every descriptor row, x / (||x|| + 1e-8), into the workspace
//                     (knn.hip: one wave per row, the bits of k_row_normalize).
//   k_seq_gate        one workgroup per query row i.  Candidates are taken 16 at a time.  The
//                     A operand of a pass is one 32-row MFMA block: rows 0 .. 2w are
//                     Xn[i - w .. i + w].  The B operand has 16 columns per candidate:
//                     columns 0 .. 2w of candidate j are Xn[j - w .. j + w].  Window rows
//                     past the ends of the map are clamped copies; the rows / columns past
//                     2w and the columns of a slot that is not a candidate are zeros.  No
//                     score reads any of those.  The product runs on v_mfma_f32_32x32x2_f32
//                     with sim_tile's staging and k order (knn.hip: slabs of 16 k, zeros
//                     past D), so element (a, c) has the bits k_sim_f32 gives
//                     S(i - w + a, j - w + c): an element's chain does not depend on where
//                     in a tile it sits.  Only each candidate's diagonal (dir +1) and
//                     anti-diagonal (dir -1) leave the accumulators, into LDS.  Then one
//                     wave, a lane per slot (hence k <= 64), applies the validity rule, the
//                     float64 sums, the direction choice and the threshold, and adds the
//                     row's judged-and-rejected count to the total with one integer atomic.
#include <limits.h>

#include "common.h"
#include "kernels.h"
#include "ws_carve.h"

namespace {

constexpr int QBK = 16;       // sim_tile's k slab (knn.hip SBK)
constexpr int SQ_KMAX = 64;   // a lane per slot
constexpr int SQ_WMAX = 7;    // 2 w + 1 <= 15 window rows in a 16-column group
constexpr int SQ_PASS = 16;   // candidates per pass: 256 B columns = 8 MFMA column blocks, 2 per wave
constexpr int SQ_COLS = SQ_PASS * 16;

// four k of a row from kx on: zeros for a dead row (p == nullptr) and past D, as sim_tile stages them
__device__ __forceinline__ float4 seq_load4(const float* __restrict__ p, int kx, int D, bool vec) {
    if (!p) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec && kx + 3 < D) return *reinterpret_cast<const float4*>(p + kx);
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = kx + u < D ? p[kx + u] : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// Three workgroups per CU: the kernel waits on its gather, so residency
// is what hides it; four would spill.
__global__ __launch_bounds__(256, 3) void k_seq_gate(const float* __restrict__ Xn, int N, int D,
                                                  const double* __restrict__ t, const int64_t* __restrict__ code,
                                                  const uint8_t* __restrict__ has, int q0, int k,
                                                  const int32_t* __restrict__ idx, const float* __restrict__ sim,
                                                  const uint8_t* __restrict__ mask, const int32_t* __restrict__ count,
                                                  int w, double min_gap, int min_terms, double thr,
                                                  double* __restrict__ s_score, int8_t* __restrict__ s_dir,
                                                  int32_t* __restrict__ s_terms, uint8_t* __restrict__ keep,
                                                  unsigned long long* __restrict__ rejected) {
    __shared__ float As[QBK][32 + 4];
    __shared__ float Bs[QBK][SQ_COLS + 4];
    __shared__ int sj[SQ_KMAX];             // the slot's frame j, or -1: not a candidate
    __shared__ float dg[2][SQ_KMAX][16];    // [dir +1 / -1][slot][a]: S(i - w + a, j + dir (a - w))
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x, i = q0 + r;
    const size_t row0 = (size_t)r * k;
    if (tid < SQ_KMAX) {
        const int cnt = min(max(count[r], 0), k);
        int j = -1;
        if (tid < cnt && (!mask || mask[row0 + tid] != 0)) {
            j = idx[row0 + tid];
            if (j < 0 || j >= N) j = -1;  // an index outside the map is never read
        }
        sj[tid] = j;
    }
    __syncthreads();
    const bool vec = (D & 3) == 0;
    const int w2 = 2 * w;
    for (int p0 = 0; p0 < k; p0 += SQ_PASS) {
        const int npass = min(SQ_PASS, k - p0);
        bool any = false;  // block-uniform: every thread reads the same slots
        for (int s = 0; s < npass; ++s) any |= sj[p0 + s] >= 0;
        if (!any) continue;
        // this thread's staging tasks: one float4 of A (threads 0 .. 127), four of B
        const float* pa = nullptr;
        const int arow = tid >> 2, akq = (tid & 3) * 4;
        if (tid < 128 && arow <= w2) pa = Xn + (size_t)min(max(i - w + arow, 0), N - 1) * D;
        const float* pb[4];
        int bcol[4], bkq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * 256;
            bcol[u] = e >> 2;
            bkq[u] = (e & 3) * 4;
            const int s = p0 + (bcol[u] >> 4), c = bcol[u] & 15;
            const int j = s < k ? sj[s] : -1;
            pb[u] = j >= 0 && c <= w2 ? Xn + (size_t)min(max(j - w + c, 0), N - 1) * D : nullptr;
        }
        // MFMA column blocks of 32 (two candidates each): block b belongs to wave b & 3
        const int nblk = (npass + 1) >> 1;
        const int nb = (int)(nblk > wave) + (int)(nblk > wave + 4);  // wave-uniform
        f32x16 acc[2];
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[tb][e] = 0.f;
        float4 va = seq_load4(pa, akq, D, vec), vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vb[u] = seq_load4(pb[u], bkq[u], D, vec);
        for (int k0 = 0; k0 < D; k0 += QBK) {
            if (tid < 128) {
                As[akq + 0][arow] = va.x; As[akq + 1][arow] = va.y;
                As[akq + 2][arow] = va.z; As[akq + 3][arow] = va.w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                Bs[bkq[u] + 0][bcol[u]] = vb[u].x; Bs[bkq[u] + 1][bcol[u]] = vb[u].y;
                Bs[bkq[u] + 2][bcol[u]] = vb[u].z; Bs[bkq[u] + 3][bcol[u]] = vb[u].w;
            }
            __syncthreads();
            if (k0 + QBK < D) {  // the next slab, in flight under the MFMAs
                va = seq_load4(pa, k0 + QBK + akq, D, vec);
#pragma unroll
                for (int u = 0; u < 4; ++u) vb[u] = seq_load4(pb[u], k0 + QBK + bkq[u], D, vec);
            }
#pragma unroll
            for (int kk = 0; kk < QBK; kk += 2) {
                const int kx = kk + (lane >> 5);
                const float a = As[kx][lane & 31];
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    if (tb < nb) {
                        const float b = Bs[kx][(wave + 4 * tb) * 32 + (lane & 31)];
                        acc[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tb], 0, 0, 0);
                    }
            }
            __syncthreads();
        }
        // D[a][col]: col = lane & 31, a = (e & 3) + 8 (e >> 2) + 4 (lane >> 5); a < 16 is e < 8
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
            if (tb < nb) {
                const int col = lane & 31, c = col & 15;
                const int s = p0 + (wave + 4 * tb) * 2 + (col >> 4);  // < p0 + 16 <= 64
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int a = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    if (a <= w2) {
                        if (a == c) dg[0][s][a] = acc[tb][e];
                        if (a == w2 - c) dg[1][s][a] = acc[tb][e];
                    }
                }
            }
    }
    __syncthreads();
    if (wave != 0) return;
    const int s = lane;
    const int j = sj[s];
    const bool cand = s < k && j >= 0;
    double score = 0.0;
    int dir = 0, terms = 0;
    bool kp = false, judged = false;
    if (cand) {
        const float g = sim[row0 + s];
        double sc[2];
        int n[2];
        const bool hi = has[i] != 0, hj = has[j] != 0;
        const int64_t ci = code[i], cj = code[j];
#pragma unroll
        for (int dd = 0; dd < 2; ++dd) {
            const int sg = dd ? -1 : 1;
            double sum = 0.0;
            int cnt = 0;
            for (int d = -w; d <= w; ++d) {
                if (d == 0) continue;
                const int ii = i + d, jj = j + sg * d;
                if (ii < 0 || ii >= N || jj < 0 || jj >= N) continue;
                if (fabs(t[ii] - t[jj]) < min_gap) continue;
                if (hi && has[ii] != 0 && code[ii] != ci) continue;
                if (hj && has[jj] != 0 && code[jj] != cj) continue;
                sum += (double)dg[dd][s][d + w];
                ++cnt;
            }
            sc[dd] = ((double)g + sum) / (double)(1 + cnt);
            n[dd] = cnt;
        }
        const bool e0 = n[0] >= min_terms, e1 = n[1] >= min_terms;
        if (!e0 && !e1) {  // kept unjudged
            score = (double)g;
            kp = true;
        } else {
            const int dd = e1 && (!e0 || sc[1] > sc[0]) ? 1 : 0;  // +1 on a tie
            score = sc[dd];
            dir = dd ? -1 : 1;
            terms = n[dd];
            kp = score >= thr;
            judged = true;
        }
    }
    if (s < k) {
        s_score[row0 + s] = score;
        s_dir[row0 + s] = (int8_t)dir;
        s_terms[row0 + s] = terms;
        keep[row0 + s] = kp ? 1 : 0;
    }
    const unsigned long long rej = __ballot(judged && !kp);
    if (rejected && lane == 0 && rej) atomicAdd(rejected, (unsigned long long)__popcll(rej));
}

struct SeqBufs {
    float* Xn;  // normalised descriptors [N, D]
};

bool seq_shape_ok(int N, int D, int Q, int k) {
    return N > 0 && D > 0 && Q > 0 && k >= 1 && k <= SQ_KMAX && (long long)Q * k <= INT_MAX;
}

size_t seq_carve(int N, int D, void* base, SeqBufs* out) {
    WsCarver c(base);
    SeqBufs b;
    b.Xn = c.take<float>((size_t)N * D);
    if (out) *out = b;
    return c.total();
}

}  // namespace

size_t mlg_seq_ws_bytes(int N, int D, int Q, int k) {
    if (!seq_shape_ok(N, D, Q, k)) return 0;
    return seq_carve(N, D, nullptr, nullptr);
}

int mlg_seq_run(const float* desc, int N, int D, const double* t, const int64_t* floor, const uint8_t* has_floor,
                int q0, int Q, int k, const int32_t* idx, const float* sim, const uint8_t* mask, const int32_t* count,
                int radius, double min_gap, int min_terms, double threshold, void* ws, size_t ws_bytes,
                double* s_score, int8_t* s_dir, int32_t* s_terms, uint8_t* keep, unsigned long long* rejected,
                hipStream_t s) {
    if (!desc || !t || !floor || !has_floor || !idx || !sim || !count || !ws || !s_score || !s_dir || !s_terms || !keep)
        return MLG_EINVAL;
    if (!seq_shape_ok(N, D, Q, k) || radius < 1 || radius > SQ_WMAX || min_terms < 1 || q0 < 0
        || (long long)q0 + Q > N)
        return MLG_EINVAL;
    SeqBufs b;
    if (seq_carve(N, D, ws, &b) > ws_bytes) return MLG_ENOMEM;
    MLG_TRY(mlg_row_normalize_wave(desc, b.Xn, N, D, nullptr, s));
    hipLaunchKernelGGL(k_seq_gate, dim3(Q), dim3(256), 0, s, b.Xn, N, D, t, floor, has_floor, q0, k, idx, sim, mask,
                       count, radius, min_gap, min_terms, threshold, s_score, s_dir, s_terms, keep, rejected);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
