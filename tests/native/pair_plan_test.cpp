// CPU check of csrc/pair_plan.h, the pair matchers' host scheduling: hand-computed tables
// for each planner and a seeded random sweep of the per-layer decision.  Built with
// -fsanitize=address,undefined by tests/test_pair_plan_cpu.py; exit status 0 = all passed.
#include <stdio.h>

#include <random>

#include "pair_plan.h"

using namespace pair_plan;

static int g_fail = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++g_fail;                                             \
        }                                                         \
    } while (0)

static bool eq(const Task& t, int a, int b, int c, int d) {
    return t.q_off == a && t.q_len == b && t.kv_off == c && t.kv_len == d;
}
static bool eq(const Move& m, int a, int b, int c, int d) {
    return m.src_off == a && m.src_len == b && m.dst_off == c && m.flag == d;
}
static bool eq(const Seg& s, int off, int len, int frame) {
    return s.off == off && s.len == len && s.frame == frame && s.pad == 0;
}

// P = 4, counts {70, 0, 64, big, 1}, pairs (0,2) (1,2) (3,4) (2,0): pair 1 has an empty
// side.  big = 130 pads to 192 rows ((130 + 63) & ~63), big = 194 to 256; `o` = the six
// expected segment offsets, `fo` the four frame offsets.
static void layout_case(int big, const int (&o)[6], int npad, const int (&fo)[4], int npadf) {
    const int32_t counts[5] = {70, 0, 64, big, 1}, pa[4] = {0, 1, 3, 2}, pb[4] = {2, 2, 4, 0};
    Segments lay;
    CHECK(lay.build(counts, pa, pb, 4, big));
    CHECK(lay.segs.size() == 6 && lay.Npad == npad);
    CHECK((lay.pair_of == std::vector<int>{0, 2, 3}));
    CHECK((lay.orig_total == std::vector<int>{134, 64, big + 1, 134}));
    const int len[6] = {70, 64, big, 1, 64, 70}, frame[6] = {0, 2, 3, 4, 2, 0};
    for (int k = 0; k < 6; ++k) CHECK(eq(lay.segs[k], o[k], len[k], frame[k]));

    AttnTables att;
    att.build(lay.segs);
    CHECK(att.tasks.size() == 12 && att.out_off.size() == 12 && att.maxq == big);
    for (int k = 0; k < 6; ++k) CHECK(eq(att.tasks[k], o[k], len[k], o[k], len[k]));  // self, segment order
    CHECK(eq(att.tasks[6], o[0], 70, o[1], 64));                                       // cross a -> b, b -> a
    CHECK(eq(att.tasks[7], o[1], 64, o[0], 70));
    CHECK(eq(att.tasks[8], o[2], big, o[3], 1));
    CHECK(eq(att.tasks[9], o[3], 1, o[2], big));
    CHECK(eq(att.tasks[10], o[4], 64, o[5], 70));
    CHECK(eq(att.tasks[11], o[5], 70, o[4], 64));
    for (int k = 0; k < 12; ++k) CHECK(att.out_off[k] == o[k % 6]);

    // frames 0, 2, 3, 4 in first-appearance order; 0 and 2 repeat
    FramePlan fp;
    fp.build(lay.segs, 4);
    CHECK(fp.repeats && fp.fsegs.size() == 4 && fp.tasks.size() == 4 && fp.out_off.size() == 4 && fp.moves.size() == 6);
    const int flen[4] = {70, 64, big, 1}, fframe[4] = {0, 2, 3, 4}, fof[6] = {0, 1, 2, 3, 1, 0};
    for (int f = 0; f < 4; ++f) {
        CHECK(eq(fp.fsegs[f], fo[f], flen[f], fframe[f]));
        CHECK(eq(fp.tasks[f], fo[f], flen[f], fo[f], flen[f]));
        CHECK(fp.out_off[f] == fo[f]);
    }
    for (int k = 0; k < 6; ++k) CHECK(eq(fp.moves[k], o[k], len[k], fo[fof[k]], 0));
    CHECK(fp.NpadF == npadf && fp.maxqf == big);
    CHECK(fp.tok == 135.0 + big);
    CHECK(fp.work == 1024.0 * (70 * 70 + 64 * 64 + big * big + 1));
}

static void test_segments_and_tables() {
    // 130 pads to 192: 192 + 192 = 384 (the layouts' padding is (len + 63) & ~63)
    layout_case(130, {0, 128, 192, 384, 448, 512}, 640, {0, 128, 192, 384}, 448);
    // the same pairs with a count that pads to 256
    layout_case(194, {0, 128, 192, 448, 512, 576}, 704, {0, 128, 192, 448}, 512);

    Segments lay;
    const int32_t pa[1] = {0}, pb[1] = {1};
    const int32_t neg[2] = {-1, 5}, big[2] = {5, 131}, edge[2] = {130, 130};
    CHECK(!lay.build(neg, pa, pb, 1, 130));
    CHECK(!lay.build(big, pa, pb, 1, 130));
    CHECK(lay.build(edge, pa, pb, 1, 130) && lay.segs.size() == 2 && lay.Npad == 384);
    // all pairs empty: an empty plan
    const int32_t c0[3] = {0, 9, 0}, qa[2] = {0, 1}, qb[2] = {1, 2};
    CHECK(lay.build(c0, qa, qb, 2, 130));
    CHECK(lay.segs.empty() && lay.pair_of.empty() && lay.Npad == 0);
    CHECK((lay.orig_total == std::vector<int>{9, 9}));
    AttnTables att;
    att.build(lay.segs);
    CHECK(att.tasks.empty() && att.out_off.empty() && att.maxq == 0);
}

static void test_distinct() {
    const int32_t ids[5] = {5, 2, 5, 7, 2};
    const Distinct d = distinct_frames(ids, 5);
    CHECK((d.unique == std::vector<int32_t>{5, 2, 7}));
    CHECK((d.index == std::vector<int32_t>{0, 1, 0, 2, 1}));
    CHECK(d.repeats());
    const int32_t all[4] = {9, -3, 0, 4};
    const Distinct e = distinct_frames(all, 4);
    CHECK(!e.repeats() && e.unique.size() == 4 && (e.index == std::vector<int32_t>{0, 1, 2, 3}));
    const Distinct z = distinct_frames(nullptr, 0);
    CHECK(!z.repeats() && z.unique.empty() && z.index.empty());

    // a single pair of two distinct frames: the per-frame stage is skipped
    const int32_t counts[2] = {10, 20}, pa[1] = {0}, pb[1] = {1};
    Segments lay;
    CHECK(lay.build(counts, pa, pb, 1, 64));
    FramePlan fp;
    fp.build(lay.segs, 4);
    CHECK(!fp.repeats && fp.tasks.empty() && fp.moves.empty());
    // the same frame on both sides repeats
    const int32_t pc[1] = {1};
    CHECK(lay.build(counts, pc, pb, 1, 64));
    fp.build(lay.segs, 4);
    CHECK(fp.repeats && fp.fsegs.size() == 1 && fp.moves.size() == 2 && fp.NpadF == 64 && fp.maxqf == 20);
    CHECK(eq(fp.moves[0], 0, 20, 0, 0) && eq(fp.moves[1], 64, 20, 0, 0));
}

// pairs (lens[2 p], lens[2 p + 1]) of distinct frames
static Segments pairs_of(const std::vector<int>& lens) {
    std::vector<int32_t> counts(lens.begin(), lens.end()), pa, pb;
    for (size_t p = 0; p < lens.size() / 2; ++p) {
        pa.push_back((int32_t)(2 * p));
        pb.push_back((int32_t)(2 * p + 1));
    }
    Segments lay;
    CHECK(lay.build(counts.data(), pa.data(), pb.data(), (int)pa.size(), 2048));
    return lay;
}

// stats = {low, kept} per segment
static void test_layer_decision() {
    LayerDecision d;
    {  // (a) nothing stops, every kept count equals len: continue, no upload
        const Segments lay = pairs_of({100, 80, 50, 60});
        const int st[8] = {100, 100, 80, 80, 50, 50, 60, 60};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.01f, 10, 0);
        CHECK(!d.changed() && d.stopped.empty() && !d.any_prune && d.moves.empty() && d.stop_layer.empty());
    }
    {  // (b) the middle one of three pairs is confident: stopped, the others re-packed from 0
        const Segments lay = pairs_of({100, 80, 50, 60, 70, 30});  // offsets 0 128 256 320 384 512
        const int st[12] = {100, 100, 80, 80, 0, 50, 0, 60, 70, 70, 30, 30};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.01f, 1024, 2);
        CHECK(d.changed() && !d.any_prune && (d.stopped == std::vector<size_t>{2}));
        CHECK((d.pair_of == std::vector<int>{0, 2}) && d.segs.size() == 4 && d.Npad == 448);
        CHECK(eq(d.segs[0], 0, 100, 0) && eq(d.segs[1], 128, 80, 1) && eq(d.segs[2], 256, 70, 4) &&
              eq(d.segs[3], 384, 30, 5));
        CHECK(d.moves.size() == 4 && eq(d.moves[0], 0, 100, 0, 1) && eq(d.moves[1], 128, 80, 128, 1) &&
              eq(d.moves[2], 384, 70, 256, 1) && eq(d.moves[3], 512, 30, 384, 1));
        CHECK(d.stop_layer.empty());
    }
    {  // (c) len = pruning_min + 1 with kept < len is gathered; len = pruning_min is copied whole
        const Segments lay = pairs_of({41, 40});
        const int st[4] = {41, 30, 40, 20};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.01f, 40, 1);
        CHECK(d.changed() && d.any_prune && d.stopped.empty());
        CHECK(d.moves.size() == 2 && eq(d.moves[0], 0, 41, 0, 0) && eq(d.moves[1], 64, 40, 64, 1));
        CHECK(d.segs.size() == 2 && eq(d.segs[0], 0, 30, 0) && eq(d.segs[1], 64, 40, 1) && d.Npad == 128);
        // ... and alone it does not count as pruned
        const Segments lay2 = pairs_of({40, 40});
        const int st2[4] = {40, 10, 40, 10};
        d.decide(lay2.segs, lay2.pair_of, lay2.orig_total, st2, 0.95f, 0.01f, 40, 1);
        CHECK(!d.changed() && !d.any_prune && d.moves.empty());
    }
    {  // (d) a side pruned to nothing: the pair is removed, stop_layer = i + 2
        const Segments lay = pairs_of({50, 60, 50, 60});
        const int st[8] = {50, 0, 60, 55, 50, 50, 60, 60};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.01f, 10, 3);
        CHECK(d.changed() && d.any_prune && d.stopped.empty() && d.moves.size() == 4);
        CHECK(eq(d.moves[0], 0, 50, 0, 0) && eq(d.moves[1], 64, 60, 0, 0) && eq(d.moves[2], 128, 50, 64, 0) &&
              eq(d.moves[3], 192, 60, 128, 0));
        CHECK((d.pair_of == std::vector<int>{1}) && d.segs.size() == 2 && eq(d.segs[0], 64, 50, 2) &&
              eq(d.segs[1], 128, 60, 3) && d.Npad == 192);
        CHECK(d.stop_layer.size() == 1 && d.stop_layer[0] == std::make_pair(0, 5));
    }
    {  // (e) depth_conf <= 0 never stops, width_conf <= 0 never prunes
        const Segments lay = pairs_of({50, 60});
        const int st[4] = {0, 10, 0, 10};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.f, 0.f, 10, 0);
        CHECK(!d.changed());
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, -1.f, 0.01f, 10, 0);
        CHECK(d.stopped.empty() && d.any_prune && d.segs.size() == 2 && d.segs[0].len == 10);
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.f, 10, 0);
        CHECK((d.stopped == std::vector<size_t>{0}) && !d.any_prune);
    }
    {  // (f) every pair stopped: empty layout, Npad = 64, no moves
        const Segments lay = pairs_of({50, 60, 70, 80});
        const int st[8] = {0, 50, 0, 60, 1, 70, 0, 80};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.01f, 10, 4);
        CHECK(d.changed() && (d.stopped == std::vector<size_t>{0, 2}));
        CHECK(d.segs.empty() && d.pair_of.empty() && d.moves.empty() && d.Npad == 64 && d.stop_layer.empty());
    }
    {  // (g) the comparison is `>`: 1.0f - 10.f / 200.f is exactly 0.95f and does not stop; 9 low tokens do
        CHECK(1.0f - 10.f / 200.f == 0.95f);
        const Segments lay = pairs_of({100, 100});
        const int st[4] = {5, 100, 5, 100};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st, 0.95f, 0.01f, 1024, 0);
        CHECK(d.stopped.empty() && !d.changed());
        const int st2[4] = {5, 100, 4, 100};
        d.decide(lay.segs, lay.pair_of, lay.orig_total, st2, 0.95f, 0.01f, 1024, 0);
        CHECK((d.stopped == std::vector<size_t>{0}) && d.changed());
    }
}

static void test_random_sweep() {
    std::mt19937 rng(20240607);
    auto pick = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    const float depths[3] = {0.f, 0.5f, 0.95f}, widths[2] = {0.f, 0.01f};
    const int mins[3] = {0, 50, 1024};
    for (int it = 0; it < 200; ++it) {
        const int P = pick(1, 6), F = pick(2, 8);
        std::vector<int32_t> counts(F), pa(P), pb(P);
        for (int& c : counts) c = pick(0, 9) == 0 ? 0 : pick(1, 200);
        for (int p = 0; p < P; ++p) {
            pa[p] = pick(0, F - 1);
            pb[p] = pick(0, F - 1);
        }
        Segments lay;
        CHECK(lay.build(counts.data(), pa.data(), pb.data(), P, 200));
        AttnTables att;
        att.build(lay.segs);
        CHECK(att.tasks.size() == 2 * lay.segs.size() && att.out_off.size() == 2 * lay.segs.size());
        FramePlan fp;
        fp.build(lay.segs, 4);
        for (const Move& m : fp.moves) CHECK(m.dst_off % 64 == 0 && m.dst_off + pad64(m.src_len) <= fp.NpadF);
        std::vector<int> stats;
        for (const Seg& g : lay.segs) {
            stats.push_back(pick(0, g.len));
            stats.push_back(pick(0, 3) == 0 ? g.len : pick(0, g.len));
        }
        LayerDecision d;
        d.decide(lay.segs, lay.pair_of, lay.orig_total, stats.data(), depths[pick(0, 2)], widths[pick(0, 1)],
                 mins[pick(0, 2)], pick(0, 7));
        const size_t np = lay.segs.size() / 2;
        CHECK(d.stopped.size() <= np && d.Npad % 64 == 0 && d.Npad >= 64);
        if (!d.changed()) {
            CHECK(d.moves.empty() && d.segs.empty());
            continue;
        }
        CHECK(d.moves.size() == 2 * (np - d.stopped.size()));
        CHECK(d.segs.size() == 2 * d.pair_of.size() && d.pair_of.size() + d.stop_layer.size() == np - d.stopped.size());
        int end = 0;  // rows used so far
        for (size_t k = 0; k < d.segs.size(); k += 2) {
            const Seg a = d.segs[k], b = d.segs[k + 1];
            CHECK(a.off % 64 == 0 && b.off % 64 == 0 && a.len > 0 && b.len > 0);
            CHECK(a.off >= end && (k == 0 || a.off > d.segs[k - 1].off));  // increasing, no overlap
            CHECK(b.off == a.off + pad64(a.len));                         // adjacent, (a, b) order
            end = b.off + pad64(b.len);
        }
        CHECK(end <= d.Npad);
    }
}

int main() {
    test_segments_and_tables();
    test_distinct();
    test_layer_decision();
    test_random_sweep();
    if (g_fail) {
        printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("pair_plan: all checks passed\n");
    return 0;
}
