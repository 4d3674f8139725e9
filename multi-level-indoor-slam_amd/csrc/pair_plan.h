// Host scheduling of the pair matchers: which rows every kernel of a call touches.
//
// LightGlue and SuperGlue lay all images of all pairs of a call out in ONE flat token
// layout: segment 2k (image a of the k-th active pair) and 2k + 1 (image b), each padded to
// a multiple of 64 rows.  This header turns (counts, pairs) into that layout, the layout
// into the ragged attention's task tables, LightGlue's layer 0 into a per-frame layout, and
// a layer's statistics into the next, compacted layout.  Plain C++17, no HIP: the drivers
// (lightglue.hip, superglue.hip, loftr.hip) upload the tables and launch; a CPU program
// (tests/native/pair_plan_test.cpp) checks them under the sanitizers.
//
// LIFETIME RULE.  The plan objects own their tables as pageable std::vectors, and the
// drivers upload them with hipMemcpyAsync.  Such a copy may read its source until the
// stream reaches it, so a table that has been uploaded must not be rebuilt, moved from or
// destroyed before the stream has been synchronised.  The drivers keep every plan object
// at function scope, call build() / decide() again only right after a synchronisation
// (LightGlue: the per-layer statistics read-back) and synchronise once more before
// returning.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "ws_carve.h"

namespace pair_plan {

struct Seg {
    int off, len, frame, pad;  // flat row offset, live tokens, source frame, unused
};
// one ragged-attention task: queries [q_off, q_off + q_len) attend to keys / values
// [kv_off, kv_off + kv_len); the kernels read it as int4 (.x .y .z .w)
struct Task {
    int q_off, q_len, kv_off, kv_len;
};
// one row move: LightGlue's compaction (rows src_off + i -> dst_off + rank(i); flag 0:
// the rows of the keep mask, flag 1: all of them) and its layer-0 frame -> segment copy
// (segment src_off / src_len <- frame rows from dst_off); read as int4 as well
struct Move {
    int src_off, src_len, dst_off, flag;
};
static_assert(sizeof(Seg) == 16 && sizeof(Task) == 16 && sizeof(Move) == 16, "tables are uploaded by bytes");
static_assert(offsetof(Task, q_off) == 0 && offsetof(Task, q_len) == 4 && offsetof(Task, kv_off) == 8 &&
                  offsetof(Task, kv_len) == 12,
              "Task is the kernels' int4");
static_assert(offsetof(Move, src_off) == 0 && offsetof(Move, src_len) == 4 && offsetof(Move, dst_off) == 8 &&
                  offsetof(Move, flag) == 12,
              "Move is the kernels' int4");

inline int pad64(int n) { return (n + 63) & ~63; }

// The distinct ids of a list in first-appearance order, and each entry's index into them.
struct Distinct {
    std::vector<int32_t> unique, index;
    bool repeats() const { return unique.size() < index.size(); }
};
inline Distinct distinct_frames(const int32_t* ids, size_t n) {
    Distinct d;
    d.index.resize(n);
    std::unordered_map<int32_t, int32_t> pos;
    for (size_t g = 0; g < n; ++g) {
        auto it = pos.find(ids[g]);
        if (it == pos.end()) {
            it = pos.emplace(ids[g], (int32_t)d.unique.size()).first;
            d.unique.push_back(ids[g]);
        }
        d.index[g] = it->second;
    }
    return d;
}

// Pair p -> segments [a | b]; a pair with an empty side gets none (no matches, as the
// reference's early exit).
struct Segments {
    std::vector<Seg> segs;
    std::vector<int> pair_of;     // the caller's pair index per active segment pair
    std::vector<int> orig_total;  // tokens of both images, per caller pair
    int Npad = 0;                 // rows of the layout

    // false: a count outside [0, kmax]
    bool build(const int32_t* counts, const int32_t* pa, const int32_t* pb, int P, int kmax) {
        segs.clear();
        pair_of.clear();
        orig_total.assign(P > 0 ? P : 0, 0);
        Npad = 0;
        for (int p = 0; p < P; ++p) {
            const int la = counts[pa[p]], lb = counts[pb[p]];
            if (la < 0 || la > kmax || lb < 0 || lb > kmax) return false;
            orig_total[p] = la + lb;
            if (la == 0 || lb == 0) continue;
            segs.push_back(Seg{Npad, la, pa[p], 0});
            Npad += pad64(la);
            segs.push_back(Seg{Npad, lb, pb[p], 0});
            Npad += pad64(lb);
            pair_of.push_back(p);
        }
        return true;
    }
};

// The ragged attention's tables of a layout: self tasks (seg -> seg) in segment order,
// then the cross tasks (a -> b, b -> a per pair); task t writes its context rows from
// out_off[t] (the query segment's offset).
struct AttnTables {
    std::vector<Task> tasks;
    std::vector<int> out_off;
    int maxq = 0;

    void build(const std::vector<Seg>& segs) {
        tasks.clear();
        out_off.clear();
        maxq = 0;
        for (const Seg& g : segs) {
            tasks.push_back(Task{g.off, g.len, g.off, g.len});
            maxq = std::max(maxq, g.len);
        }
        for (size_t k = 0; k + 1 < segs.size(); k += 2) {
            const Seg a = segs[k], b = segs[k + 1];
            tasks.push_back(Task{a.off, a.len, b.off, b.len});
            tasks.push_back(Task{b.off, b.len, a.off, a.len});
        }
        for (int rep = 0; rep < 2; ++rep)
            for (const Seg& g : segs) out_off.push_back(g.off);
    }
};

// LightGlue layer 0's self block reads one image only, so it runs once per distinct frame
// of the call on a frame layout; `moves` then copy each frame's rows into every pair
// segment of that frame.  Nothing but `repeats` is built when no frame repeats (the stage
// is skipped).
struct FramePlan {
    std::vector<Seg> fsegs;
    std::vector<Task> tasks;  // self tasks of the frame layout
    std::vector<int> out_off;
    std::vector<Move> moves;  // per pair segment: (segment off, len, its frame's off, 0)
    int NpadF = 0, maxqf = 0;
    double tok = 0, work = 0;  // profiling: live tokens, attention FLOPs (4 heads q kv 64)
    bool repeats = false;

    void build(const std::vector<Seg>& segs, int heads) {
        fsegs.clear();
        tasks.clear();
        out_off.clear();
        moves.clear();
        NpadF = maxqf = 0;
        tok = work = 0;
        std::vector<int32_t> ids;
        for (const Seg& g : segs) ids.push_back(g.frame);
        const Distinct d = distinct_frames(ids.data(), ids.size());
        repeats = d.repeats();
        if (!repeats) return;
        int foff = 0;
        for (size_t k = 0; k < segs.size(); ++k)
            if ((size_t)d.index[k] == fsegs.size()) {  // the frame's first appearance
                fsegs.push_back(Seg{foff, segs[k].len, segs[k].frame, 0});
                foff += pad64(segs[k].len);
            }
        NpadF = std::max(foff, 64);
        for (const Seg& f : fsegs) {
            tasks.push_back(Task{f.off, f.len, f.off, f.len});
            out_off.push_back(f.off);
            maxqf = std::max(maxqf, f.len);
            tok += f.len;
            work += 4.0 * heads * 64 * (double)f.len * f.len;
        }
        for (size_t k = 0; k < segs.size(); ++k)
            moves.push_back(Move{segs[k].off, segs[k].len, fsegs[d.index[k]].off, 0});
    }
};

// LightGlue after layer i: stats[2 k] = tokens of segment k with confidence below the
// layer's threshold, stats[2 k + 1] = tokens its pruning mask keeps.  A pair whose confident
// ratio exceeds depth_conf stops (its assignment runs at this layer); of the others, a
// segment longer than pruning_min is pruned to its kept tokens; the survivors are packed
// from row 0.
struct LayerDecision {
    std::vector<size_t> stopped;  // index (in the old layout) of image a's segment of each stopped pair
    bool any_prune = false;
    std::vector<Move> moves;      // old segment -> new offset, for every segment of a pair not stopped
    std::vector<Seg> segs;        // the new layout (pairs with a side pruned to nothing dropped)
    std::vector<int> pair_of;
    int Npad = 64;
    std::vector<std::pair<int, int>> stop_layer;  // (caller's pair, layer) of pairs ended by pruning

    bool changed() const { return !stopped.empty() || any_prune; }  // else: same layout, nothing to upload

    void decide(const std::vector<Seg>& old, const std::vector<int>& old_pair_of, const std::vector<int>& orig_total,
                const int* stats, float depth_conf, float width_conf, int pruning_min, int i) {
        stopped.clear();
        any_prune = false;
        moves.clear();
        segs.clear();
        pair_of.clear();
        stop_layer.clear();
        std::vector<char> stop(old.size() / 2, 0);
        for (size_t k = 0; k + 1 < old.size(); k += 2) {
            const int p = old_pair_of[k / 2];
            if (depth_conf > 0.f) {
                const float low = (float)(stats[2 * k] + stats[2 * k + 2]);
                const float ratio = 1.0f - low / (float)orig_total[p];
                if (ratio > depth_conf) {
                    stop[k / 2] = 1;
                    stopped.push_back(k);
                }
            }
            if (!stop[k / 2] && width_conf > 0.f)
                for (int q = 0; q < 2; ++q)
                    if (old[k + q].len > pruning_min && stats[2 * (k + q) + 1] != old[k + q].len) any_prune = true;
        }
        int noff = 0;
        if (changed())
            for (size_t k = 0; k + 1 < old.size(); k += 2) {
                if (stop[k / 2]) continue;
                Seg n[2];
                for (int q = 0; q < 2; ++q) {
                    const Seg sg = old[k + q];
                    const bool prune = width_conf > 0.f && sg.len > pruning_min;
                    const int nl = prune ? stats[2 * (k + q) + 1] : sg.len;
                    moves.push_back(Move{sg.off, sg.len, noff, prune ? 0 : 1});
                    n[q] = Seg{noff, nl, sg.frame, 0};
                    noff += pad64(nl);
                }
                // an empty side after pruning ends that pair with no matches (reference loop break)
                if (n[0].len == 0 || n[1].len == 0) {
                    stop_layer.emplace_back(old_pair_of[k / 2], i + 2);
                    continue;
                }
                segs.push_back(n[0]);
                segs.push_back(n[1]);
                pair_of.push_back(old_pair_of[k / 2]);
            }
        Npad = std::max(noff, 64);
    }
};

}  // namespace pair_plan

#ifdef __HIPCC__
// live[r] = row r is a live token of some segment; with a RowSeg (`int*`) argument also
// rowseg[r] = that segment, or -1.  SuperGlue instantiates it without one.  Segments are in
// increasing offset order: binary search for the last one starting at or before r (a
// linear scan over every segment per row was quadratic).
template <typename... RowSeg>
__global__ void k_pair_live(const pair_plan::Seg* __restrict__ segs, int nseg, uint8_t* __restrict__ live,
                            RowSeg __restrict__... rowseg, int Npad) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= Npad) return;
    int lo = 0, hi = nseg - 1, sgi = -1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].off <= r) {
            sgi = mid;
            lo = mid + 1;
        } else {
            hi = mid - 1;
        }
    }
    if (sgi >= 0 && r >= segs[sgi].off + segs[sgi].len) sgi = -1;
    live[r] = sgi >= 0;
    ((rowseg[r] = sgi), ...);
}
#endif
