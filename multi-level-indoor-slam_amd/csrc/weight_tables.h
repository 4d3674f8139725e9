// One table per weight struct of include/mlgate.h, in the order of the flat tensor list the
// operators of torch_ops.cpp take for it, and the one function that fills a struct from such a
// list.  The table is the list order: entry i names the field tensor i lands in, its element
// kind and the element count of the layout documented beside the field in mlgate.h.
// The DINOv2 ViT list is described once (add_vit); ViT-B's vit_table is that description at
// (768, 12) over mlg_vit_weights, dino_table the same over mlg_dino_weights at any hub width.
// Plain C++17 over mlgate.h, model_shapes.h and the standard library (no torch, no HIP), so
// tests/native/weight_tables_test.cpp checks it stand-alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/mlgate.h"
#include "model_shapes.h"

namespace wt {

enum Kind : int8_t { BF16, F32, U8, OTHER };  // OTHER: a descriptor of any other element type

inline const char* kind_name(Kind k) {
    switch (k) {
        case BF16: return "bf16";
        case F32: return "f32";
        case U8: return "u8";
        default: return "another dtype";
    }
}

struct Entry {
    size_t offset;  // offsetof the pointer field
    Kind kind;
    bool optional;  // an empty tensor is accepted and stored as NULL
    int64_t numel;
    char name[24];  // e.g. "self[3].Wf1"
};
using Table = std::vector<Entry>;

// what the filler needs to know of tensor i
struct Desc {
    const void* ptr;
    Kind kind;
    int64_t numel;
    int device;  // -1 = host
    bool contiguous;
};

constexpr bool OPTIONAL = true;

inline void add(Table& t, size_t offset, const std::string& name, Kind kind, int64_t numel, bool optional = false) {
    Entry e{offset, kind, optional, numel, {0}};
    snprintf(e.name, sizeof e.name, "%s", name.c_str());
    t.push_back(e);
}
inline std::string at(const char* array, int i) { return std::string(array) + "[" + std::to_string(i) + "]"; }

// n pointers from `offset` on, one list entry each, named "array[i]"; numel: one count for
// all of them, or a function of i
template <class N>
inline void add_array(Table& t, size_t offset, const char* array, int n, Kind kind, N numel, bool optional = false) {
    for (int i = 0; i < n; ++i) {
        int64_t count;
        if constexpr (std::is_invocable_v<N, int>) count = numel(i);
        else count = numel;
        add(t, offset + i * sizeof(void*), at(array, i), kind, count, optional);
    }
}

// Field `f` of struct T lying at byte `base` (0, or an array element's offset), named pre + "f":
// WT_FIELD(t, base, pre, T, f, kind, numel [, wt::OPTIONAL])
#define WT_FIELD(t, base, pre, T, f, ...) wt::add(t, (base) + offsetof(T, f), std::string(pre) + #f, __VA_ARGS__)
// The n pointers of array field `f` of struct T: WT_ARRAY(t, T, f, n, kind, numel [, wt::OPTIONAL])
#define WT_ARRAY(t, T, f, n, ...) wt::add_array(t, offsetof(T, f), #f, n, __VA_ARGS__)

// A table is built on first use, by `build`, and kept: one per call site ...
template <class F>
inline const Table& built_once(F build) {
    static const Table tab = [&] {
        Table t;
        build(t);
        return t;
    }();
    return tab;
}
// ... or one per value of the parameters its sizes depend on
template <class Key, class F>
inline const Table& built_once_per(const Key& key, F build) {
    static std::mutex mu;
    static std::map<Key, Table> tabs;  // a map's elements stay where they are
    const std::lock_guard<std::mutex> lock(mu);
    auto it = tabs.find(key);
    if (it == tabs.end()) {
        it = tabs.emplace(key, Table()).first;
        build(it->second);
    }
    return it->second;
}

// rows of a split-packed GEMM weight with n output rows: the split GEMM's 256-column tile
// (mlgate.h: zero rows up to the next multiple of 256; only ViT-S has such weights)
inline int64_t split_rows(int64_t n) { return (n + 255) / 256 * 256; }

// The one description of a DINOv2 ViT list: patch_w, patch_b, cls, pos, `depth` x the fourteen
// fields of mlg_vit_block, norm_w, norm_b, for a network of width E.  W holds the six net-level
// fields (mlg_vit_weights or mlg_dino_weights) and lies at byte `base`; block 0 lies at byte
// `blocks`.  split: MLG_VIT_SPLIT packing ([W_hi | W_lo]: 2x the GEMM weights, rows padded to
// split_rows); tokens = 1 + (S/14)^2
template <class W>
inline void add_vit(Table& t, size_t base, size_t blocks, bool split, int64_t tokens, int64_t E, int depth) {
    using B = mlg_vit_block;
    const int64_t m = split ? 2 : 1;
    const auto rows = [=](int64_t n) { return split ? split_rows(n) : n; };
    WT_FIELD(t, base, "", W, patch_w, BF16, rows(E) * MLG_VIT_PATCH_K * m);
    WT_FIELD(t, base, "", W, patch_b, F32, E);
    WT_FIELD(t, base, "", W, cls, F32, E);
    WT_FIELD(t, base, "", W, pos, F32, tokens * E);
    for (int i = 0; i < depth; ++i) {
        const size_t o = blocks + i * sizeof(B);
        const std::string p = at("blocks", i) + ".";
        WT_FIELD(t, o, p, B, norm1_w, F32, E);
        WT_FIELD(t, o, p, B, norm1_b, F32, E);
        WT_FIELD(t, o, p, B, qkv_w, BF16, rows(3 * E) * E * m);
        WT_FIELD(t, o, p, B, qkv_b, F32, 3 * E);
        WT_FIELD(t, o, p, B, proj_w, BF16, rows(E) * E * m);
        WT_FIELD(t, o, p, B, proj_b, F32, E);
        WT_FIELD(t, o, p, B, ls1, F32, E);
        WT_FIELD(t, o, p, B, norm2_w, F32, E);
        WT_FIELD(t, o, p, B, norm2_b, F32, E);
        WT_FIELD(t, o, p, B, fc1_w, BF16, rows(4 * E) * E * m);
        WT_FIELD(t, o, p, B, fc1_b, F32, 4 * E);
        WT_FIELD(t, o, p, B, fc2_w, BF16, rows(E) * 4 * E * m);
        WT_FIELD(t, o, p, B, fc2_b, F32, E);
        WT_FIELD(t, o, p, B, ls2, F32, E);
    }
    WT_FIELD(t, base, "", W, norm_w, F32, E);
    WT_FIELD(t, base, "", W, norm_b, F32, E);
}

// ViT-B/14 over mlg_vit_weights: the general description at (768, 12), its blocks inline
inline const Table& vit_table(bool split, int64_t tokens) {
    return built_once_per(std::make_pair(split, tokens), [=](Table& t) {
        add_vit<mlg_vit_weights>(t, 0, offsetof(mlg_vit_weights, blocks), split, tokens, MLG_VIT_EMBED, MLG_VIT_DEPTH);
    });
}

// mlg_dino_weights with the block array it points to behind it, so that one table addresses
// both; after wt::fill, set w.blocks = blocks
struct DinoFlat {
    mlg_dino_weights w;
    mlg_vit_block blocks[MLG_DINO_MAX_DEPTH];
};

// the network of width `embed` and `depth` blocks, over DinoFlat
inline const Table& dino_table(bool split, int64_t tokens, int64_t embed, int depth) {
    return built_once_per(std::make_tuple(split, tokens, embed, depth), [=](Table& t) {
        add_vit<mlg_dino_weights>(t, offsetof(DinoFlat, w), offsetof(DinoFlat, blocks), split, tokens, embed,
                                  depth < MLG_DINO_MAX_DEPTH ? depth : MLG_DINO_MAX_DEPTH);
    });
}

inline const Table& salad_table() {
    return built_once([](Table& t) {
        using W = mlg_salad_weights;
        WT_FIELD(t, 0, "", W, w1, BF16, 1024 * MLG_VIT_EMBED);
        WT_FIELD(t, 0, "", W, b1, F32, 1024);
        WT_FIELD(t, 0, "", W, w2, BF16, 256 * 1024);
        WT_FIELD(t, 0, "", W, b2, F32, 256);
        WT_FIELD(t, 0, "", W, wt1, F32, 512 * MLG_VIT_EMBED);
        WT_FIELD(t, 0, "", W, bt1, F32, 512);
        WT_FIELD(t, 0, "", W, wt2, F32, 256 * 512);
        WT_FIELD(t, 0, "", W, bt2, F32, 256);
    });
}

// CricaVPR's cross-image encoder: 2 nn.TransformerEncoderLayer, GEMM weights [W_hi | W_lo]
inline const Table& crica_table() {
    return built_once([](Table& t) {
        using W = mlg_crica_weights;
        using L = mlg_crica_layer;
        const int64_t E = MLG_VIT_EMBED, F = 2048;
        for (int i = 0; i < 2; ++i) {
            const size_t o = offsetof(W, layers) + i * sizeof(L);
            const std::string p = at("layers", i) + ".";
            WT_FIELD(t, o, p, L, in_w, BF16, 3 * E * 2 * E);
            WT_FIELD(t, o, p, L, in_b, F32, 3 * E);
            WT_FIELD(t, o, p, L, out_w, BF16, E * 2 * E);
            WT_FIELD(t, o, p, L, out_b, F32, E);
            WT_FIELD(t, o, p, L, ln1_g, F32, E);
            WT_FIELD(t, o, p, L, ln1_b, F32, E);
            WT_FIELD(t, o, p, L, fc1_w, BF16, F * 2 * E);
            WT_FIELD(t, o, p, L, fc1_b, F32, F);
            WT_FIELD(t, o, p, L, fc2_w, BF16, E * 2 * F);
            WT_FIELD(t, o, p, L, fc2_b, F32, E);
            WT_FIELD(t, o, p, L, ln2_g, F32, E);
            WT_FIELD(t, o, p, L, ln2_b, F32, E);
        }
    });
}

inline const Table& sp_table() {
    return built_once([](Table& t) {
        using W = mlg_sp_weights;
        WT_FIELD(t, 0, "", W, conv1a_w, F32, 64 * 9);
        WT_FIELD(t, 0, "", W, conv1a_b, F32, 64);
        WT_ARRAY(t, W, w, 11, BF16, [](int i) {
            const SpLayer l = SP_LAYERS[i];
            return (int64_t)l.cout * l.k * l.k * l.cin;
        });
        WT_ARRAY(t, W, b, 11, F32, [](int i) { return SP_LAYERS[i].cout; });
    });
}

// One mlg_lg_block at offset o: LightGlue's (qkv_rows 768 self / 512 cross, with the FFN's
// LayerNorm) or a SuperGlue layer (with_ln false: ln_g / ln_b are unused and not in its list)
inline void add_lg_block(Table& t, size_t o, int qkv_rows, bool with_ln, const std::string& p) {
    using B = mlg_lg_block;
    WT_FIELD(t, o, p, B, Wqkv, BF16, qkv_rows * 256);
    WT_FIELD(t, o, p, B, bqkv, F32, qkv_rows);
    WT_FIELD(t, o, p, B, Wout, BF16, 256 * 256);
    WT_FIELD(t, o, p, B, bout, F32, 256);
    WT_FIELD(t, o, p, B, Wf1, BF16, 512 * 512);
    WT_FIELD(t, o, p, B, bf1, F32, 512);
    if (with_ln) {
        WT_FIELD(t, o, p, B, ln_g, F32, 512);
        WT_FIELD(t, o, p, B, ln_b, F32, 512);
    }
    WT_FIELD(t, o, p, B, Wf2, BF16, 256 * 512);
    WT_FIELD(t, o, p, B, bf2, F32, 256);
}

inline const Table& lg_table() {
    return built_once([](Table& t) {
        using W = mlg_lg_weights;
        const size_t B = sizeof(mlg_lg_block);
        WT_FIELD(t, 0, "", W, Wr, F32, 32 * 2);
        for (int i = 0; i < 9; ++i) add_lg_block(t, offsetof(W, self) + i * B, 768, true, at("self", i) + ".");
        for (int i = 0; i < 9; ++i) add_lg_block(t, offsetof(W, cross) + i * B, 512, true, at("cross", i) + ".");
        WT_ARRAY(t, W, Wfinal, 9, BF16, 256 * 256);
        WT_ARRAY(t, W, bfinal, 9, F32, 256);
        WT_ARRAY(t, W, wmatch, 9, F32, 256);
        WT_ARRAY(t, W, bmatch, 9, F32, 1);
        WT_ARRAY(t, W, wconf, 8, F32, 256);
        WT_ARRAY(t, W, bconf, 8, F32, 1);
        WT_FIELD(t, 0, "", W, ones, F32, 256);
    });
}

inline const Table& sg_table() {
    return built_once([](Table& t) {
        using W = mlg_sg_weights;
        const int kenc[4] = {3, 32, 64, 128};  // KeypointEncoder MLP channels up to kenc_w4's input
        WT_ARRAY(t, W, kenc_w, 3, F32, [&](int i) { return kenc[i + 1] * kenc[i]; });
        WT_ARRAY(t, W, kenc_b, 3, F32, [&](int i) { return kenc[i + 1]; });
        WT_FIELD(t, 0, "", W, kenc_w4, BF16, 256 * 128);
        WT_FIELD(t, 0, "", W, kenc_b4, F32, 256);
        WT_FIELD(t, 0, "", W, kenc_w5, BF16, 256 * 256);
        WT_FIELD(t, 0, "", W, kenc_b5, F32, 256);
        for (int i = 0; i < 18; ++i)
            add_lg_block(t, offsetof(W, layer) + i * sizeof(mlg_lg_block), 768, false, at("layer", i) + ".");
        WT_FIELD(t, 0, "", W, Wfinal, BF16, 256 * 256);
        WT_FIELD(t, 0, "", W, bfinal, F32, 256);
    });
}

// stem_w, stem_b and the bottlenecks of the first `stages` ResNet-50 stages of struct W
// (mlg_rn_weights: 4 stages; mlg_mixvpr_weights: 3)
template <class W>
inline void add_rn_trunk(Table& t, int stages) {
    using B = mlg_rn_block;
    WT_FIELD(t, 0, "", W, stem_w, F32, 64 * 7 * 7 * 3);
    WT_FIELD(t, 0, "", W, stem_b, F32, 64);
    int64_t cin = 64;
    int blk = 0;
    for (int st = 0; st < stages; ++st) {
        const int64_t width = RN_WIDTHS[st], wpad = width < 128 ? 128 : width;
        for (int bi = 0; bi < RN_NBLOCKS[st]; ++bi, ++blk) {
            const size_t o = offsetof(W, blocks) + blk * sizeof(B);
            const std::string p = at("blocks", blk) + ".";
            WT_FIELD(t, o, p, B, w1, BF16, wpad * cin);
            WT_FIELD(t, o, p, B, b1, F32, wpad);
            WT_FIELD(t, o, p, B, w2, BF16, wpad * 9 * width);
            WT_FIELD(t, o, p, B, b2, F32, wpad);
            WT_FIELD(t, o, p, B, w3, BF16, 4 * width * width);
            WT_FIELD(t, o, p, B, b3, F32, 4 * width);
            // the downsample conv belongs to a stage's first block; elsewhere an empty tensor = NULL
            WT_FIELD(t, o, p, B, wd, BF16, 4 * width * cin, bi != 0);
            WT_FIELD(t, o, p, B, bd, F32, 4 * width, bi != 0);
            cin = 4 * width;
        }
    }
}

inline const Table& rn_table() {
    return built_once([](Table& t) {
        add_rn_trunk<mlg_rn_weights>(t, RN_STAGES);
    });
}

inline const Table& mixvpr_trunk_table() {
    return built_once([](Table& t) {
        add_rn_trunk<mlg_mixvpr_weights>(t, 3);
    });
}

inline const Table& mixvpr_head_table() {
    return built_once([](Table& t) {
        using W = mlg_mixvpr_weights;
        WT_FIELD(t, 0, "", W, mix_w, BF16, 4 * 2 * 26 * 416 * 16);
        WT_FIELD(t, 0, "", W, mix_p, F32, 4 * 4 * 512);
        WT_FIELD(t, 0, "", W, row_w, F32, 4 * 512);
        WT_FIELD(t, 0, "", W, chan_w, F32, 1024 * 1024);
        WT_FIELD(t, 0, "", W, chan_b, F32, 1024);
        WT_FIELD(t, 0, "", W, row_s, F32, 4);
        WT_FIELD(t, 0, "", W, row_b, F32, 4);
    });
}

// tails_bytes > 0: the list ends with the packed coarse tails (mlg_loftr_tails_bytes() of u8)
inline const Table& loftr_table(int64_t tails_bytes) {
    return built_once_per(tails_bytes, [=](Table& t) {
        using W = mlg_loftr_weights;
        using L = mlg_loftr_layer;
        WT_FIELD(t, 0, "", W, stem_w, F32, 49 * 128);
        WT_FIELD(t, 0, "", W, stem_b, F32, 128);
        WT_ARRAY(t, W, conv_w, MLG_LOFTR_NCONV, BF16, [](int i) {
            const ConvSpec c = CONVS[i];
            return (int64_t)c.cout * c.k * c.k * c.cin;
    });
    // no bias for the convs without BatchNorm
    WT_ARRAY(t, W, conv_b, MLG_LOFTR_NCONV, F32, [](int i) { return CONVS[i].cout; }, OPTIONAL);
    for (int l = 0; l < 10; ++l) {
        const bool coarse = l < 8;
        const int64_t d = coarse ? 256 : 128;
        const int i = coarse ? l : l - 8;
        const size_t o = (coarse ? offsetof(W, coarse) : offsetof(W, fine)) + i * sizeof(L);
        const std::string p = at(coarse ? "coarse" : "fine", i) + ".";
        WT_FIELD(t, o, p, L, w, BF16, 3 * d * d);
        WT_FIELD(t, o, p, L, wmerge, BF16, d * d);
        WT_FIELD(t, o, p, L, w1, BF16, 2 * d * 2 * d);
        WT_FIELD(t, o, p, L, w2, BF16, d * 2 * d);
        WT_FIELD(t, o, p, L, ln1_g, F32, d);
        WT_FIELD(t, o, p, L, ln1_b, F32, d);
        WT_FIELD(t, o, p, L, ln2_g, F32, d);
        WT_FIELD(t, o, p, L, ln2_b, F32, d);
    }
    WT_FIELD(t, 0, "", W, down_w, BF16, 128 * 256);
    WT_FIELD(t, 0, "", W, down_b, F32, 128);
    WT_FIELD(t, 0, "", W, merge_wf, BF16, 128 * 128);
    WT_FIELD(t, 0, "", W, merge_wc, BF16, 128 * 128);
    WT_FIELD(t, 0, "", W, merge_b, F32, 128);
    if (tails_bytes > 0) WT_FIELD(t, 0, "", W, coarse_tails, U8, tails_bytes, OPTIONAL);
    });
}

// Fill the pointer fields of `strukt` (one of the structs `table` was built for) from the n
// tensors d[0..n).  Tensor i passes if it is on the device d[0] is on, contiguous, of the
// entry's kind and element count and, for bf16, 16-byte aligned; an optional entry also takes
// an empty tensor of any kind (stored as NULL).  Returns "" and writes every field, or the
// first failure (index, field, expected, found) and writes nothing.
inline std::string fill(const Table& table, const char* model, const Desc* d, size_t n, void* strukt) {
    char msg[320];
    if (n != table.size()) {
        snprintf(msg, sizeof msg, "%s weights: expected %zu tensors, got %zu", model, table.size(), n);
        return msg;
    }
    for (size_t i = 0; i < n; ++i) {
        const Entry& e = table[i];
        const Desc& t = d[i];
        const char* found = nullptr;
        char buf[96];
        if (t.device != d[0].device) {
            snprintf(buf, sizeof buf, "a tensor on device %d", t.device);
            found = t.device < 0 ? "a host tensor" : buf;
        } else if (e.optional && t.numel == 0) {
            continue;
        } else if (t.kind != e.kind) {
            found = kind_name(t.kind);
        } else if (t.numel != e.numel) {
            snprintf(buf, sizeof buf, "%lld elements", (long long)t.numel);
            found = buf;
        } else if (!t.contiguous) {
            found = "a non-contiguous view";
        } else if (e.kind == BF16 && (reinterpret_cast<uintptr_t>(t.ptr) & 15)) {
            found = "a pointer that is not 16-byte aligned";
        }
        if (found) {
            char where[48];
            snprintf(where, sizeof where, "device %d", d[0].device);
            snprintf(msg, sizeof msg, "%s weights[%zu] (%s): expected %s%s with %lld elements, contiguous, on %s as "
                     "weights[0]; got %s", model, i, e.name, e.optional ? "empty or " : "", kind_name(e.kind),
                     (long long)e.numel, d[0].device < 0 ? "the host" : where, found);
            return msg;
        }
    }
    for (size_t i = 0; i < n; ++i)
        *reinterpret_cast<const void**>(static_cast<char*>(strukt) + table[i].offset) = d[i].numel ? d[i].ptr : nullptr;
    return "";
}

}  // namespace wt
