// JPEG keyframe ingestion, host half: the sorted(*.jpg) files of
// process_image_sequence (place_recognition.py:960-973) -> quantised DCT coefficients.
//
// Huffman decoding is a serial bit stream, so one image is one job on the same kind of
// thread pool as the PNG decoder (ingest.cpp); everything after it -- dequantisation,
// the inverse DCT, chroma upsampling, colour conversion -- is independent integer
// arithmetic per block / pixel and runs on the GPU (jpeg.hip).  What this file writes
// per image is therefore not pixels but int16 coefficients in natural order, the
// quantisation tables and a small record of block counts and offsets (include/mlgate.h).
//
// Only what cv2.imread decodes to the same pixels through the device half is accepted;
// every other stream gets a status and stays with the legacy reader (mlgate/ingest.py).
// The parser is stricter than libjpeg on damaged streams (libjpeg pads a truncated scan
// with zeros and resynchronises on restart markers): anything it would warn about is
// MLG_EINVAL here.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

#include "../../include/mlgate.h"

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined = false;
    uint8_t counts[17] = {0};
    uint8_t syms[256] = {0};
    // 9-bit lookahead: (length << 8) | symbol, 0 when the code is longer than 9 bits
    uint16_t look[512];
    int32_t maxcode[18];  // largest code of each length, -1 if none
    int32_t valoff[17];
    int nsyms = 0;
};

// Canonical code assignment (ITU T.81 annex C); false if the counts do not form a prefix code.
bool build_huff(Huff& h) {
    std::memset(h.look, 0, sizeof h.look);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = p - code;
        for (int i = 0; i < h.counts[l]; ++i, ++p, ++code) {
            if (code >= (1 << l)) return false;
            if (l <= 9) {
                const int first = code << (9 - l);
                for (int k = 0; k < (1 << (9 - l)); ++k) h.look[first + k] = (uint16_t)(l << 8 | h.syms[p]);
            }
        }
        h.maxcode[l] = h.counts[l] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    return true;
}

struct Comp {
    int id = 0, h = 0, v = 0, tq = 0, td = 0, ta = 0;
};

struct Jpeg {
    int width = 0, height = 0, ncomp = 0;
    Comp comp[4];
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = 0, orientation = 0 /* 0: no tag */, restart = 0;
    int unsupported = 0;  // a reason was seen: the stream is valid but outside the accepted set
    bool qdef[4] = {false, false, false, false};
    uint16_t q[4][64];
    Huff dc[4], ac[4];
    size_t scan = 0;  // offset of the entropy-coded data
};

int be16(const uint8_t* p) { return p[0] << 8 | p[1]; }

// Orientation (tag 0x0112) of IFD0 of an Exif APP1 payload; 0 when absent or malformed.
int exif_orientation(const uint8_t* d, size_t n) {
    if (n < 14 || std::memcmp(d, "Exif\0\0", 6) != 0) return 0;
    const uint8_t* t = d + 6;
    const size_t tn = n - 6;
    const bool le = t[0] == 'I' && t[1] == 'I';
    if (!le && !(t[0] == 'M' && t[1] == 'M')) return 0;
    auto r16 = [&](size_t o) { return le ? t[o] | t[o + 1] << 8 : t[o] << 8 | t[o + 1]; };
    auto r32 = [&](size_t o) {
        return le ? (uint32_t)t[o] | (uint32_t)t[o + 1] << 8 | (uint32_t)t[o + 2] << 16 | (uint32_t)t[o + 3] << 24
                  : (uint32_t)t[o] << 24 | (uint32_t)t[o + 1] << 16 | (uint32_t)t[o + 2] << 8 | (uint32_t)t[o + 3];
    };
    if (r16(2) != 42) return 0;
    const size_t ifd = r32(4);
    if (ifd > tn || tn - ifd < 2) return 0;
    const size_t cnt = (size_t)r16(ifd);
    for (size_t k = 0; k < cnt; ++k) {
        const size_t e = ifd + 2 + 12 * k;
        if (e + 12 > tn) return 0;
        if (r16(e) == 0x0112) return r16(e + 8);
    }
    return 0;
}

// Marker walk up to and including SOS.  MLG_EINVAL: not a JPEG header; otherwise MLG_OK
// with j.unsupported set when the stream is outside the accepted set.
int parse(const uint8_t* d, size_t n, Jpeg& j) {
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return MLG_EINVAL;
    size_t o = 2;
    for (;;) {
        if (o >= n || d[o] != 0xFF) return MLG_EINVAL;
        while (o < n && d[o] == 0xFF) ++o;  // fill bytes
        if (o >= n) return MLG_EINVAL;
        const int m = d[o++];
        if (m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD9)) return MLG_EINVAL;  // no segment may stand here
        if (n - o < 2) return MLG_EINVAL;
        const size_t len = (size_t)be16(d + o);
        if (len < 2 || len > n - o) return MLG_EINVAL;
        const uint8_t* b = d + o + 2;
        const size_t bl = len - 2;
        o += len;
        if (m == 0xC0 || m == 0xC1) {
            if (j.have_sof || bl < 6) return MLG_EINVAL;
            const int prec = b[0];
            j.height = be16(b + 1);
            j.width = be16(b + 3);
            j.ncomp = b[5];
            if (j.width == 0 || j.ncomp == 0 || bl != 6 + 3 * (size_t)j.ncomp) return MLG_EINVAL;
            if (prec == 12 || j.height == 0) j.unsupported = 1;  // 12 bit; height by DNL
            else if (prec != 8) return MLG_EINVAL;
            if (j.ncomp > 4) return MLG_EINVAL;
            for (int c = 0; c < j.ncomp; ++c) {
                Comp& k = j.comp[c];
                k.id = b[6 + 3 * c];
                k.h = b[7 + 3 * c] >> 4;
                k.v = b[7 + 3 * c] & 15;
                k.tq = b[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) return MLG_EINVAL;
            }
            j.have_sof = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            // progressive, lossless, differential and arithmetic frames: valid JPEG, not ours
            if (j.have_sof || bl < 6) return MLG_EINVAL;
            j.height = be16(b + 1);
            j.width = be16(b + 3);
            j.ncomp = b[5];
            j.have_sof = true;
            j.unsupported = 1;
            if (j.ncomp >= 1 && j.ncomp <= 4 && bl >= 6 + 3 * (size_t)j.ncomp) {
                j.comp[0].h = b[7] >> 4;
                j.comp[0].v = b[7] & 15;
            }
            return MLG_OK;  // nothing past this frame header is read
        } else if (m == 0xCC) {  // DAC: arithmetic conditioning
            j.unsupported = 1;
        } else if (m == 0xC4) {
            size_t p = 0;
            while (p < bl) {
                if (bl - p < 17) return MLG_EINVAL;
                const int tc = b[p] >> 4, th = b[p] & 15;
                if (tc > 1 || th > 3) return MLG_EINVAL;
                Huff& h = tc ? j.ac[th] : j.dc[th];
                int total = 0;
                h.counts[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (h.counts[l] = b[p + l]);
                p += 17;
                h.defined = false;
                if (total > 256 || (size_t)total > bl - p) return MLG_EINVAL;
                std::memset(h.syms, 0, sizeof h.syms);
                std::memcpy(h.syms, b + p, (size_t)total);
                p += (size_t)total;
                h.nsyms = total;
                if (!build_huff(h)) return MLG_EINVAL;
                if (!tc)
                    for (int i = 0; i < total; ++i)
                        if (h.syms[i] > 15) return MLG_EINVAL;  // a DC category is at most 15 bits
                h.defined = true;
            }
        } else if (m == 0xDB) {
            size_t p = 0;
            while (p < bl) {
                const int pq = b[p] >> 4, tq = b[p] & 15;
                if (pq > 1 || tq > 3) return MLG_EINVAL;
                const size_t need = pq ? 128 : 64;
                if (bl - p - 1 < need) return MLG_EINVAL;
                for (int k = 0; k < 64; ++k)
                    j.q[tq][kZigzag[k]] = (uint16_t)(pq ? be16(b + p + 1 + 2 * k) : b[p + 1 + k]);
                j.qdef[tq] = true;
                p += 1 + need;
            }
        } else if (m == 0xDD) {
            if (bl != 2) return MLG_EINVAL;
            j.restart = be16(b);
        } else if (m == 0xE0) {
            if (bl >= 12 && std::memcmp(b, "JFIF\0", 5) == 0) j.jfif = true;
        } else if (m == 0xE1) {
            const int ori = exif_orientation(b, bl);
            if (ori) j.orientation = ori;
        } else if (m == 0xEE) {
            if (bl >= 12 && std::memcmp(b, "Adobe", 5) == 0) {
                j.adobe = true;
                j.adobe_transform = b[11];
            }
        } else if (m == 0xDA) {
            if (!j.have_sof || bl < 1) return MLG_EINVAL;
            const int ns = b[0];
            if (ns < 1 || ns > 4 || bl != 4 + 2 * (size_t)ns) return MLG_EINVAL;
            if (ns != j.ncomp) {
                j.unsupported = 1;  // one scan per component
            } else {
                for (int c = 0; c < ns; ++c) {
                    if (b[1 + 2 * c] != j.comp[c].id) j.unsupported = 1;  // another component order
                    j.comp[c].td = b[2 + 2 * c] >> 4;
                    j.comp[c].ta = b[2 + 2 * c] & 15;
                    if (j.comp[c].td > 3 || j.comp[c].ta > 3) return MLG_EINVAL;
                }
            }
            j.scan = o;
            break;
        }
        // every other segment (COM, APPn, DNL, ...) is skipped by its length
    }
    // colour space and sampling, by libjpeg's rules restricted to what the device half does
    if (j.orientation != 0 && j.orientation != 1) j.unsupported = 1;
    if (j.ncomp == 3) {
        const bool ycc = j.jfif || (j.adobe && j.adobe_transform == 1);
        if (!ycc) j.unsupported = 1;
        const Comp* c = j.comp;
        if (c[1].h != 1 || c[1].v != 1 || c[2].h != 1 || c[2].v != 1) j.unsupported = 1;
        if (!((c[0].h == 1 && c[0].v == 1) || (c[0].h == 2 && c[0].v == 1) || (c[0].h == 2 && c[0].v == 2)))
            j.unsupported = 1;
    } else if (j.ncomp != 1) {
        j.unsupported = 1;
    }
    return MLG_OK;
}

// Block grid of an accepted stream: ncomp 1 (sampling normalised to 1x1: a single-component
// scan is not interleaved, its MCU is one block) or 3 with luma h x v over 1x1 chroma.
struct Grid {
    int ncomp, h, v, mcux, mcuy;
    int bcols[3], brows[3];
    size_t off[3], total;  // int16 elements
};

Grid grid_of(int ncomp, int h, int v, int H, int W) {
    Grid g{};
    g.ncomp = ncomp;
    g.h = ncomp == 1 ? 1 : h;
    g.v = ncomp == 1 ? 1 : v;
    g.mcux = (W + 8 * g.h - 1) / (8 * g.h);
    g.mcuy = (H + 8 * g.v - 1) / (8 * g.v);
    size_t o = 0;
    for (int c = 0; c < ncomp; ++c) {
        g.bcols[c] = g.mcux * (c ? 1 : g.h);
        g.brows[c] = g.mcuy * (c ? 1 : g.v);
        g.off[c] = o;
        o += (size_t)g.bcols[c] * g.brows[c] * 64;
    }
    g.total = o;
    return g;
}

// Entropy-coded segment reader: byte stuffing (FF 00), fill bytes, and a stop at the next
// marker, after which zero bits are fed (`fake` counts them, always the newest bits).
struct Bits {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int n = 0, fake = 0;
    bool marker = false;

    void fill() {
        while (n <= 56) {
            unsigned b = 0;
            if (!marker) {
                if (p >= end) {
                    marker = true;
                } else if (*p != 0xFF) {
                    b = *p++;
                } else {
                    const uint8_t* q = p + 1;
                    while (q < end && *q == 0xFF) ++q;
                    if (q < end && *q == 0) {
                        b = 0xFF;
                        p = q + 1;
                    } else {
                        marker = true;  // p stays on the marker's FF
                    }
                }
            }
            if (marker) fake += 8;
            acc = acc << 8 | b;
            n += 8;
        }
    }
    inline unsigned peek(int k) { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1); }
    inline void skip(int k) { n -= k; }
    // true once bits that were never in the file have been consumed
    bool overrun() const { return n < fake; }
    void reset() {
        acc = 0;
        n = fake = 0;
        marker = false;
    }
};

inline int decode_sym(Bits& br, const Huff& h) {
    if (br.n < 16) br.fill();
    const unsigned lk = h.look[br.peek(9)];
    if (lk) {
        br.skip(lk >> 8);
        return lk & 255;
    }
    const int code16 = (int)br.peek(16);
    for (int l = 10; l <= 16; ++l) {
        const int code = code16 >> (16 - l);
        if (code <= h.maxcode[l]) {
            br.skip(l);
            return h.syms[(code + h.valoff[l]) & 255];
        }
    }
    return -1;
}

inline int receive_extend(Bits& br, int s) {
    if (br.n < s) br.fill();
    const int x = (int)br.peek(s);
    br.skip(s);
    return x < (1 << (s - 1)) ? x - (1 << s) + 1 : x;
}

// One block into `blk` (zeroed here).  DC prediction wraps like JCOEF (unsigned arithmetic).
inline bool decode_block(Bits& br, const Huff& dc, const Huff& ac, uint32_t& pred, int16_t* blk) {
    std::memset(blk, 0, 128);
    int s = decode_sym(br, dc);
    if (s < 0) return false;
    if (s) pred += (uint32_t)receive_extend(br, s);
    blk[0] = (int16_t)(uint16_t)pred;
    for (int k = 1; k < 64; ++k) {
        s = decode_sym(br, ac);
        if (s < 0) return false;
        const int r = s >> 4;
        s &= 15;
        if (s) {
            k += r;
            if (k > 63) return false;
            blk[kZigzag[k]] = (int16_t)receive_extend(br, s);
        } else {
            if (r != 15) break;
            k += 15;
        }
    }
    return true;
}

int decode_into(const uint8_t* d, size_t n, int16_t* coefs, uint16_t* qtabs, int32_t* params, int H, int W) {
    std::memset(params, 0, MLG_JPEG_PARAMS * sizeof(int32_t));
    if (!d) return MLG_EINVAL;
    Jpeg j;
    const int rc = parse(d, n, j);
    if (rc != MLG_OK) return rc;
    if (j.unsupported) return MLG_EUNSUP;
    for (int c = 0; c < j.ncomp; ++c)
        if (!j.qdef[j.comp[c].tq] || !j.dc[j.comp[c].td].defined || !j.ac[j.comp[c].ta].defined) return MLG_EINVAL;
    if (j.width != W || j.height != H) return MLG_ESIZE;
    const Grid g = grid_of(j.ncomp, j.comp[0].h, j.comp[0].v, H, W);

    Bits br{d + j.scan, d + n};
    uint32_t pred[3] = {0, 0, 0};
    const long mcus = (long)g.mcux * g.mcuy;
    int next_rst = 0;
    for (long m = 0; m < mcus; ++m) {
        if (j.restart && m && m % j.restart == 0) {
            // the interval ended: at most 7 padding bits, then RSTn in sequence
            br.fill();
            if (!br.marker || br.overrun() || br.n - br.fake > 7) return MLG_EINVAL;
            const uint8_t* q = br.p;
            while (q < br.end && *q == 0xFF) ++q;
            if (q >= br.end || *q != 0xD0 + next_rst) return MLG_EINVAL;
            next_rst = (next_rst + 1) & 7;
            br.p = q + 1;
            br.reset();
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int mx = (int)(m % g.mcux), my = (int)(m / g.mcux);
        for (int c = 0; c < g.ncomp; ++c) {
            const int hc = c ? 1 : g.h, vc = c ? 1 : g.v;
            const Huff& dc = j.dc[j.comp[c].td];
            const Huff& ac = j.ac[j.comp[c].ta];
            for (int v = 0; v < vc; ++v)
                for (int h = 0; h < hc; ++h) {
                    int16_t* blk = coefs + g.off[c] + ((size_t)(my * vc + v) * g.bcols[c] + (mx * hc + h)) * 64;
                    if (!decode_block(br, dc, ac, pred[c], blk)) return MLG_EINVAL;
                }
        }
        if (br.overrun()) return MLG_EINVAL;  // the scan ended inside this MCU
    }
    br.fill();
    if (!br.marker || br.overrun() || br.n - br.fake > 7) return MLG_EINVAL;
    const uint8_t* q = br.p;
    while (q < br.end && *q == 0xFF) ++q;
    if (q >= br.end || *q != 0xD9) return MLG_EINVAL;  // EOI must follow the scan

    std::memset(qtabs, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < g.ncomp; ++c) std::memcpy(qtabs + 64 * c, j.q[j.comp[c].tq], 128);
    params[0] = g.ncomp;
    params[1] = g.h;
    params[2] = g.v;
    for (int c = 0; c < g.ncomp; ++c) {
        params[4 + 4 * c] = g.bcols[c];
        params[5 + 4 * c] = g.brows[c];
        params[6 + 4 * c] = (int32_t)g.off[c];
    }
    return MLG_OK;
}

bool read_file(const char* path, std::vector<uint8_t>& buf) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    bool ok = std::fseek(f, 0, SEEK_END) == 0;
    const long sz = ok ? std::ftell(f) : -1;
    ok = ok && sz > 0 && std::fseek(f, 0, SEEK_SET) == 0;
    if (ok) {
        buf.resize((size_t)sz);
        ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    }
    std::fclose(f);
    return ok;
}

template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::exception&) {
        return MLG_ENOMEM;
    }
}

template <class F>
void pool(int n, int threads, F&& job) {
    threads = std::max(1, std::min(threads, n));
    std::atomic<int> next{0};
    auto worker = [&] {
        for (int i; (i = next.fetch_add(1)) < n;) job(i);
    };
    std::vector<std::thread> ts;
    for (int t = 1; t < threads; ++t) ts.emplace_back(worker);
    worker();
    for (auto& t : ts) t.join();
}

bool dims_ok(int H, int W) { return H > 0 && W > 0 && H <= 65535 && W <= 65535; }

}  // namespace

extern "C" {

int mlg_jpeg_info(const uint8_t* data, size_t len, int32_t* info) {
    if (!data || !info) return MLG_EINVAL;
    Jpeg j;
    const int rc = guarded([&] { return parse(data, len, j); });
    if (rc != MLG_OK) return rc;
    info[0] = j.width;
    info[1] = j.height;
    info[2] = j.ncomp;
    info[3] = j.comp[0].h;
    info[4] = j.comp[0].v;
    info[5] = j.unsupported ? 0 : 1;
    info[6] = info[7] = 0;
    return MLG_OK;
}

size_t mlg_jpeg_coef_bytes(int H, int W) {
    if (!dims_ok(H, W)) return 0;
    size_t worst = 0;
    static const int hv[3][2] = {{1, 1}, {2, 1}, {2, 2}};
    for (const auto& s : hv) worst = std::max(worst, grid_of(3, s[0], s[1], H, W).total);
    return worst * sizeof(int16_t);
}

int mlg_jpeg_params_check(const int32_t* params, int n, int H, int W, size_t coef_bytes) {
    if (n < 0 || !dims_ok(H, W) || (n && !params)) return MLG_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int32_t* p = params + (size_t)i * MLG_JPEG_PARAMS;
        const int nc = p[0], h = p[1], v = p[2];
        if (nc == 0) continue;  // the record of an image that was not decoded: the kernel skips it
        if (nc != 1 && nc != 3) return MLG_EINVAL;
        if (!((h == 1 && v == 1) || (nc == 3 && h == 2 && (v == 1 || v == 2)))) return MLG_EINVAL;
        const Grid g = grid_of(nc, h, v, H, W);
        for (int c = 0; c < nc; ++c) {
            const int32_t off = p[6 + 4 * c];
            if (p[4 + 4 * c] != g.bcols[c] || p[5 + 4 * c] != g.brows[c]) return MLG_EINVAL;
            if (off < 0 || off % 64) return MLG_EINVAL;
            const size_t last = ((size_t)off + (size_t)g.bcols[c] * g.brows[c] * 64) * sizeof(int16_t);
            if (last > coef_bytes) return MLG_EINVAL;
        }
    }
    return MLG_OK;
}

int mlg_jpeg_coefs_decode(const uint8_t* const* data, const size_t* lens, int n, int16_t* coefs, uint16_t* qtabs,
                          int32_t* params, int H, int W, int threads, int32_t* status) {
    if (n < 0 || !dims_ok(H, W) || (n && (!data || !lens || !coefs || !qtabs || !params || !status)))
        return MLG_EINVAL;
    const size_t stride = mlg_jpeg_coef_bytes(H, W) / sizeof(int16_t);
    pool(n, threads, [&](int i) {
        status[i] = guarded([&] {
            return decode_into(data[i], lens[i], coefs + stride * i, qtabs + 192 * (size_t)i,
                               params + MLG_JPEG_PARAMS * (size_t)i, H, W);
        });
    });
    return MLG_OK;
}

int mlg_jpeg_coefs_load(const char* const* paths, int n, int16_t* coefs, uint16_t* qtabs, int32_t* params, int H,
                        int W, int threads, int32_t* status) {
    if (n < 0 || !dims_ok(H, W) || (n && (!paths || !coefs || !qtabs || !params || !status))) return MLG_EINVAL;
    const size_t stride = mlg_jpeg_coef_bytes(H, W) / sizeof(int16_t);
    pool(n, threads, [&](int i) {
        status[i] = guarded([&] {
            std::vector<uint8_t> buf;
            if (!read_file(paths[i], buf)) {
                std::memset(params + MLG_JPEG_PARAMS * (size_t)i, 0, MLG_JPEG_PARAMS * sizeof(int32_t));
                return (int)MLG_EINVAL;
            }
            return decode_into(buf.data(), buf.size(), coefs + stride * i, qtabs + 192 * (size_t)i,
                               params + MLG_JPEG_PARAMS * (size_t)i, H, W);
        });
    });
    return MLG_OK;
}

}  // extern "C"
