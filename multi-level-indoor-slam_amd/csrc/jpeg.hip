// JPEG keyframe ingestion, device half: quantised DCT coefficients
// (csrc/jpeg.cpp) -> BGR uint8 frames, the pixels cv2.imread / libjpeg-turbo give with
// their defaults (jpeg_idct_islow, fancy upsampling, the 16-bit fixed-point YCbCr
// conversion), bit for bit.  All arithmetic is 32-bit integer, written on uint32_t so
// that hostile coefficients wrap instead of being undefined; `>>` is applied to int32_t.
//
// One kernel, one pass.  A workgroup owns a 64 x 32 tile of output pixels:
//   A  every 8x8 block the tile needs -- luma 8 x 4 blocks; chroma 8 x 4 (4:4:4), or the
//      4 x 4 (4:2:2) / 4 x 2 (4:2:0) blocks under the tile plus one halo block on each
//      side that the fancy upsampling filter reaches into -- is loaded row-wise (one 16 B
//      load per lane: a block is 128 contiguous bytes), dequantised and put into LDS;
//   B  column pass of the IDCT, one lane per column, in place in LDS;
//   C  row pass, one lane per row, + 128, clamp -> uint8 component planes in LDS;
//   D  per output pixel: chroma upsampling straight from the planes, colour conversion,
//      BGR bytes into an LDS staging row;
//   E  the staging rows go out as whole dwords (bytes only where a row's ends do not fall
//      on a dword boundary: W * 3 need not be a multiple of 4).
// The halo blocks are decoded again by the neighbouring tile (80 block IDCTs per 4:2:0 tile
// instead of 48); in exchange no component plane ever goes through HBM: traffic is the
// coefficients once (3 B / pixel at 4:2:0) plus the BGR store (3 B / pixel).
#include "../../include/mlgate.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TW = 64, TH = 32;      // output tile
constexpr int MAXBLK = 96;           // 3 components x 8 x 4 blocks
constexpr int WS_LD = 72;            // int32 words per block in LDS: 64 + 8, so the column pass
                                     // of the 4 blocks of a 32-lane group covers 32 distinct banks
constexpr int PIX_LD = TW * 3;

__device__ __forceinline__ int32_t descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// One 1-D pass of jpeg_idct_islow (CONST_BITS 13): v[0..7] -> v[0..7], descaled by `shift`.
__device__ __forceinline__ void islow_1d(uint32_t (&v)[8], int shift) {
    uint32_t z2 = v[2], z3 = v[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 + z3 * (uint32_t)-15137;
    uint32_t tmp3 = z1 + z2 * 6270u;
    z2 = v[0];
    z3 = v[4];
    uint32_t tmp0 = (z2 + z3) << 13;
    uint32_t tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7];
    tmp1 = v[5];
    tmp2 = v[3];
    tmp3 = v[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 *= (uint32_t)-7373;
    z2 *= (uint32_t)-20995;
    z3 *= (uint32_t)-16069;
    z4 *= (uint32_t)-3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    v[0] = (uint32_t)descale(tmp10 + tmp3, shift);
    v[7] = (uint32_t)descale(tmp10 - tmp3, shift);
    v[1] = (uint32_t)descale(tmp11 + tmp2, shift);
    v[6] = (uint32_t)descale(tmp11 - tmp2, shift);
    v[2] = (uint32_t)descale(tmp12 + tmp1, shift);
    v[5] = (uint32_t)descale(tmp12 - tmp1, shift);
    v[3] = (uint32_t)descale(tmp13 + tmp0, shift);
    v[4] = (uint32_t)descale(tmp13 - tmp0, shift);
}

__device__ __forceinline__ int clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// Upsampled chroma sample at output pixel (gx, gy).  `pl` is the component's LDS plane
// (64 B pitch) whose sample (0, 0) is component sample (ox, oy); cw x ch is the real
// (downsampled) component size: nothing at or beyond it is read.
__device__ __forceinline__ int chroma_at(const uint8_t* pl, int ox, int oy, int sx, int sy, int cw, int ch, int gx,
                                         int gy) {
#define S_(i, j) ((int)pl[((j) - oy) * TW + ((i) - ox)])
    if (sx == 1) return S_(gx, gy);
    const int i = gx >> 1;
    if (cw <= 2) return S_(i, sy == 2 ? gy >> 1 : gy);  // libjpeg-turbo replicates narrow components
    const bool odd = gx & 1;
    if (sy == 1) {  // h2v1 fancy: 3/4 nearer + 1/4 further
        const int a = S_(i, gy);
        if (odd) return i == cw - 1 ? a : (3 * a + S_(i + 1, gy) + 2) >> 2;
        return i == 0 ? a : (3 * a + S_(i - 1, gy) + 1) >> 2;
    }
    // h2v2 fancy: 9/16, 3/16, 3/16, 1/16 triangle; the rows past the top / bottom are the edge rows
    const int j = gy >> 1;
    const int jn = (gy & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const int s = 3 * S_(i, j) + S_(i, jn);
    if (odd) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * S_(i + 1, j) + S_(i + 1, jn) + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * S_(i - 1, j) + S_(i - 1, jn) + 8) >> 4;
#undef S_
}

__global__ __launch_bounds__(256) void k_jpeg_pixels(const int16_t* __restrict__ coefs, size_t coef_stride,
                                                     const uint16_t* __restrict__ qtabs,
                                                     const int32_t* __restrict__ params, int H, int W,
                                                     uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t ws[MAXBLK * WS_LD];
    __shared__ __attribute__((aligned(16))) uint8_t plane[3][TH * TW];
    __shared__ __attribute__((aligned(16))) uint8_t pix[TH * PIX_LD];

    const int tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y, img = blockIdx.z;
    const int32_t* P = params + (size_t)img * MLG_JPEG_PARAMS;
    const int16_t* cf = coefs + coef_stride * img;
    const uint16_t* qt = qtabs + (size_t)img * 192;
    const int nc = P[0], hmax = P[1], vmax = P[2];
    if (nc == 0) return;  // not decoded (its status says why): the frame is left as it is

    // blocks held in LDS: luma 8 x 4 from (tx * 8, ty * 4); each chroma component crw x crh
    // from (cbx0, cby0), which is one block up / left of the tile where the filter needs it
    const int hx = hmax == 2, hy = vmax == 2;
    const int crw = 8 / hmax + 2 * hx, crh = 4 / vmax + 2 * hy;
    const int cbx0 = tx * (8 / hmax) - hx, cby0 = ty * (4 / vmax) - hy;
    constexpr int NLUMA = (TW / 8) * (TH / 8);
    const int nchroma = crw * crh;
    const int nblk = NLUMA + (nc == 3 ? 2 * nchroma : 0);

    // A-C: the inverse DCT of every block, 8 lanes per block
    // (item -> block b, lane k of it; the same lane handles row k, then column k, then row k)
    for (int phase = 0; phase < 3; ++phase) {
        for (int w = tid; w < nblk * 8; w += 256) {
            const int b = w >> 3, k = w & 7;
            const int c = b < NLUMA ? 0 : (b < NLUMA + nchroma ? 1 : 2);
            const int lb = c ? b - NLUMA - (c - 1) * nchroma : b, rw = c ? crw : TW / 8;
            const int lbx = lb % rw, lby = lb / rw;
            const int bx = (c ? cbx0 : tx * (TW / 8)) + lbx, by = (c ? cby0 : ty * (TH / 8)) + lby;
            const int bcols = P[4 + 4 * c], brows = P[5 + 4 * c];
            if (bx < 0 || by < 0 || bx >= bcols || by >= brows) continue;  // outside the image: never sampled
            uint32_t* wb = ws + b * WS_LD;
            if (phase == 0) {
                const int16_t* src = cf + P[6 + 4 * c] + ((size_t)by * bcols + bx) * 64 + 8 * k;
                const uint4 cv = *reinterpret_cast<const uint4*>(src);
                const uint4 qv = *reinterpret_cast<const uint4*>(qt + 64 * c + 8 * k);
                const uint32_t cw4[4] = {cv.x, cv.y, cv.z, cv.w}, qw4[4] = {qv.x, qv.y, qv.z, qv.w};
                uint32_t d[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d[2 * e] = (uint32_t)(int32_t)(int16_t)(cw4[e] & 0xffffu) * (qw4[e] & 0xffffu);
                    d[2 * e + 1] = (uint32_t)(int32_t)(int16_t)(cw4[e] >> 16) * (qw4[e] >> 16);
                }
                *reinterpret_cast<uint4*>(wb + 8 * k) = make_uint4(d[0], d[1], d[2], d[3]);
                *reinterpret_cast<uint4*>(wb + 8 * k + 4) = make_uint4(d[4], d[5], d[6], d[7]);
            } else if (phase == 1) {
                uint32_t v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = wb[8 * e + k];
                islow_1d(v, 11);  // CONST_BITS - PASS1_BITS
#pragma unroll
                for (int e = 0; e < 8; ++e) wb[8 * e + k] = v[e];
            } else {
                const uint4 lo = *reinterpret_cast<const uint4*>(wb + 8 * k);
                const uint4 hi = *reinterpret_cast<const uint4*>(wb + 8 * k + 4);
                uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                islow_1d(v, 18);  // CONST_BITS + PASS1_BITS + 3
                uint32_t o[2];
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    o[e] = (uint32_t)clamp255((int32_t)v[4 * e] + 128) | (uint32_t)clamp255((int32_t)v[4 * e + 1] + 128) << 8 |
                           (uint32_t)clamp255((int32_t)v[4 * e + 2] + 128) << 16 |
                           (uint32_t)clamp255((int32_t)v[4 * e + 3] + 128) << 24;
                *reinterpret_cast<uint2*>(&plane[c][(lby * 8 + k) * TW + lbx * 8]) = make_uint2(o[0], o[1]);
            }
        }
        __syncthreads();
    }

    // D: upsample + colour
    const int X0 = tx * TW, Y0 = ty * TH;
    const int cw = (W + hmax - 1) / hmax, ch = (H + vmax - 1) / vmax;
    const int ox = cbx0 * 8, oy = cby0 * 8;
    for (int p = tid; p < TW * TH; p += 256) {
        const int lx = p & (TW - 1), ly = p / TW;
        const int gx = X0 + lx, gy = Y0 + ly;
        if (gx >= W || gy >= H) continue;
        const int y = plane[0][ly * TW + lx];
        int r = y, g = y, b = y;
        if (nc == 3) {
            const int cb = chroma_at(plane[1], ox, oy, hmax, vmax, cw, ch, gx, gy) - 128;
            const int cr = chroma_at(plane[2], ox, oy, hmax, vmax, cw, ch, gx, gy) - 128;
            r = clamp255(y + ((91881 * cr + 32768) >> 16));
            b = clamp255(y + ((116130 * cb + 32768) >> 16));
            g = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        }
        uint8_t* o = pix + ly * PIX_LD + lx * 3;
        o[0] = (uint8_t)b;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)r;
    }
    __syncthreads();

    // E: rows of the tile -> global, dwords where whole
    const int cols = W - X0 < TW ? W - X0 : TW;
    const size_t nb = (size_t)cols * 3;
    constexpr int WPR = PIX_LD / 4 + 1;  // dwords a 192-byte row can touch at any alignment
    for (int q = tid; q < TH * WPR; q += 256) {
        const int ly = q / WPR, kq = q % WPR;
        const int gy = Y0 + ly;
        if (gy >= H) continue;
        const size_t g0 = (((size_t)img * H + gy) * W + X0) * 3;
        const size_t a = (g0 & ~(size_t)3) + 4 * (size_t)kq;
        if (a >= g0 + nb) continue;
        const uint8_t* src = pix + ly * PIX_LD;
        if (a >= g0 && a + 4 <= g0 + nb) {
            const int s0 = (int)(a - g0);
            const uint32_t v = (uint32_t)src[s0] | (uint32_t)src[s0 + 1] << 8 | (uint32_t)src[s0 + 2] << 16 |
                               (uint32_t)src[s0 + 3] << 24;
            *reinterpret_cast<uint32_t*>(out + a) = v;
        } else {
            const size_t lo = a > g0 ? a : g0, hi = a + 4 < g0 + nb ? a + 4 : g0 + nb;
            for (size_t e = lo; e < hi; ++e) out[e] = src[e - g0];
        }
    }
}

}  // namespace

extern "C" int mlg_jpeg_pixels(const int16_t* coefs, const uint16_t* qtabs, const int32_t* params, int n, int H,
                               int W, uint8_t* out_bgr, void* stream) {
    const size_t stride = mlg_jpeg_coef_bytes(H, W);
    if (n < 0 || stride == 0) return MLG_EINVAL;
    if (n == 0) return MLG_OK;
    if (!coefs || !qtabs || !params || !out_bgr || n > 65535) return MLG_EINVAL;
    if (((uintptr_t)coefs & 15) || ((uintptr_t)qtabs & 15) || ((uintptr_t)params & 3) || ((uintptr_t)out_bgr & 3))
        return MLG_EINVAL;
    const dim3 grid((unsigned)ceil_div(W, TW), (unsigned)ceil_div(H, TH), (unsigned)n);
    hipLaunchKernelGGL(k_jpeg_pixels, grid, dim3(256), 0, (hipStream_t)stream, coefs, stride / sizeof(int16_t), qtabs,
                       params, H, W, out_bgr);
    MLG_LAUNCH_CHECK();
    return MLG_OK;
}
