// CPU check of csrc/ws_carve.h, the workspace carver every pipeline's carve function uses:
// a size-query pass (null base) and a real pass over the same takes must agree, and the
// real pass's regions must be aligned, inside the workspace and disjoint.  Each sequence is
// carved from an allocation of exactly total() bytes and every region written end to end,
// so AddressSanitizer sees an overrun.  Built with -fsanitize=address,undefined by
// tests/test_ws_carve_cpu.py; exit status 0 = all passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "ws_carve.h"

static int g_fail = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++g_fail;                                             \
        }                                                         \
    } while (0)

struct Take {
    int esize;  // 1, 2, 4, 8 or 16: the element type's size
    size_t count;
};
struct Wide {
    uint64_t a, b;
};

// the take through the element type of that size; writes every element when the pointer is real
template <class T>
static char* take_fill(WsCarver& c, size_t n, T v) {
    T* p = c.take<T>(n);
    if (p)
        for (size_t i = 0; i < n; ++i) p[i] = v;
    return reinterpret_cast<char*>(p);
}
static char* take(WsCarver& c, const Take& t, uint8_t tag) {
    const uint64_t w = 0x0101010101010101ull * tag;
    switch (t.esize) {
        case 1: return take_fill<uint8_t>(c, t.count, (uint8_t)w);
        case 2: return take_fill<uint16_t>(c, t.count, (uint16_t)w);
        case 4: return take_fill<uint32_t>(c, t.count, (uint32_t)w);
        case 8: return take_fill<uint64_t>(c, t.count, w);
        default: return take_fill<Wide>(c, t.count, Wide{w, w});
    }
}

static void run_sequence(const std::vector<Take>& seq) {
    // size query: null base, null pointers, the total
    WsCarver q(nullptr);
    size_t expect = 0;
    for (size_t i = 0; i < seq.size(); ++i) {
        CHECK(q.total() == expect);
        CHECK(take(q, seq[i], 0) == nullptr);
        expect += (seq[i].count * seq[i].esize + 255) / 256 * 256;
    }
    const size_t total = q.total();
    CHECK(total == expect && total % 256 == 0);
    if (total == 0) return;
    // the real pass over an allocation of exactly that size
    char* base = static_cast<char*>(aligned_alloc(256, total));
    CHECK(base != nullptr);
    if (!base) return;
    memset(base, 0, total);
    WsCarver c(base);
    std::vector<char*> at(seq.size());
    for (size_t i = 0; i < seq.size(); ++i) at[i] = take(c, seq[i], (uint8_t)(i % 255 + 1));
    CHECK(c.total() == total);
    for (size_t i = 0; i < seq.size(); ++i) {
        const size_t bytes = seq[i].count * seq[i].esize;
        CHECK(at[i] != nullptr && at[i] >= base && (size_t)(at[i] - base) % 256 == 0);
        CHECK((size_t)(at[i] - base) + bytes <= total);
        // a zero-count take is the position of the next one; otherwise regions are disjoint
        if (i + 1 < seq.size()) CHECK(bytes == 0 ? at[i + 1] == at[i] : at[i + 1] >= at[i] + bytes);
        // still this region's own fill after every later region was written: no overlap
        bool own = true;
        for (size_t k = 0; k < bytes; ++k) own = own && (uint8_t)at[i][k] == (uint8_t)(i % 255 + 1);
        CHECK(own);
    }
    free(base);
}

int main() {
    CHECK(a256(0) == 0 && a256(1) == 256 && a256(255) == 256 && a256(256) == 256 && a256(257) == 512);
    {  // hand-computed: f32 x 3 (12 B), nothing, u8 x 256, u16 x 129 (258 B), 16 B x 16, u64 x 33 (264 B)
        WsCarver c(nullptr);
        CHECK(c.take<float>(3) == nullptr && c.total() == 256);
        CHECK(c.take<float>(0) == nullptr && c.total() == 256);
        CHECK(c.take<uint8_t>(256) == nullptr && c.total() == 512);
        CHECK(c.take<uint16_t>(129) == nullptr && c.total() == 1024);
        CHECK(c.take<Wide>(16) == nullptr && c.total() == 1280);
        CHECK(c.take<uint64_t>(33) == nullptr && c.total() == 1792);
        run_sequence({{4, 3}, {4, 0}, {1, 256}, {2, 129}, {16, 16}, {8, 33}});
    }
    {  // a zero-count take returns the current position and does not advance
        alignas(256) static char buf[512];
        WsCarver c(buf);
        CHECK(c.take<double>(0) == (double*)buf && c.total() == 0);
        CHECK(c.take<char>(1) == buf && c.total() == 256);
        CHECK(c.take<int32_t>(0) == (int32_t*)(buf + 256) && c.total() == 256);
        CHECK(c.take<int32_t>(64) == (int32_t*)(buf + 256) && c.total() == 512);
    }
    run_sequence({});
    run_sequence({{4, 0}, {2, 0}});
    run_sequence({{1, 0}, {1, 1}, {1, 0}});
    // seeded sweep: counts whose byte size is a multiple of 256, one element over, one under, small and large
    std::mt19937 rng(12345);
    const int sizes[5] = {1, 2, 4, 8, 16};
    for (int it = 0; it < 400; ++it) {
        std::vector<Take> seq(rng() % 12);
        for (Take& t : seq) {
            t.esize = sizes[rng() % 5];
            const size_t per = 256 / t.esize, m = rng() % 9;
            switch (rng() % 6) {
                case 0: t.count = m * per; break;      // exactly m granules (m = 0: nothing)
                case 1: t.count = m * per + 1; break;  // one element over
                case 2: t.count = (m + 1) * per - 1; break;
                case 3: t.count = rng() % 4; break;
                case 4: t.count = rng() % 5000; break;
                default: t.count = 100000 + rng() % 100000; break;
            }
        }
        run_sequence(seq);
    }
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
