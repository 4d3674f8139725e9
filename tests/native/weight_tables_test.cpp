// CPU check of csrc/weight_tables.h: the tables that say which tensor of an operator's flat
// weight list lands in which field of the public weight structs (include/mlgate.h), and the
// filler behind every weighted operator of torch_ops.cpp.  For each table: the offsets are
// distinct, pointer-aligned and inside the struct, and with the 8-byte head, the scalar
// fields and the fields a list deliberately leaves out they tile sizeof(struct) exactly; the
// length is the list length the operators have always taken.  The filler writes each pointer
// at the field the table names, and every rejection fires with the index and the field name.
// Built with -fsanitize=address,undefined by tests/test_weight_tables_cpu.py; exit status 0 =
// all passed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "weight_tables.h"

static int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

struct Span {
    size_t off, size;
};
#define TAIL_FROM(T, field) Span{offsetof(T, field), sizeof(T) - offsetof(T, field)}
static const Span HEAD{0, 8};

// offsets distinct, aligned, in bounds; tables + others cover every byte of the struct once
static void check_tiling(const char* name, std::vector<const wt::Table*> tables, size_t struct_size,
                         std::vector<Span> others) {
    std::vector<int> cover(struct_size, 0);
    for (const wt::Table* t : tables)
        for (const wt::Entry& e : *t) {
            CHECK(e.offset % alignof(void*) == 0);
            CHECK(e.offset + sizeof(void*) <= struct_size);
            CHECK(e.numel > 0 && e.name[0]);
            if (e.offset + sizeof(void*) <= struct_size)
                for (size_t b = 0; b < sizeof(void*); ++b) ++cover[e.offset + b];
        }
    for (const Span& s : others) {
        CHECK(s.off + s.size <= struct_size);
        for (size_t b = 0; b < s.size && s.off + b < struct_size; ++b) ++cover[s.off + b];
    }
    size_t bad = 0;
    for (int c : cover) bad += c != 1;
    if (bad) printf("%s: %zu of %zu bytes not covered exactly once\n", name, bad, struct_size);
    CHECK(bad == 0);
}

static int find(const wt::Table& t, const char* name) {
    for (size_t i = 0; i < t.size(); ++i)
        if (!strcmp(t[i].name, name)) return (int)i;
    printf("no entry named %s\n", name);
    ++g_fail;
    return 0;
}

static const void* tag(size_t i) { return reinterpret_cast<const void*>(uintptr_t(0x10000 + 16 * i)); }

// a list the table accepts: tensor i at "address" tag(i), on device 0
static std::vector<wt::Desc> good(const wt::Table& t) {
    std::vector<wt::Desc> d;
    for (size_t i = 0; i < t.size(); ++i) d.push_back({tag(i), t[i].kind, t[i].numel, 0, true});
    return d;
}

template <class S>
static S filled(const wt::Table& t) {
    S s;
    memset(&s, 0, sizeof s);
    const std::vector<wt::Desc> d = good(t);
    const std::string err = wt::fill(t, "test", d.data(), d.size(), &s);
    if (!err.empty()) printf("unexpected: %s\n", err.c_str());
    CHECK(err.empty());
    return s;
}
#define AT(t, s, field, name) CHECK((const void*)(s).field == tag(find(t, name)))

// the filler must refuse `d`, name slot `idx` and its field, say `what`, and leave the struct alone
static void refuse(const wt::Table& t, const std::vector<wt::Desc>& d, int idx, const char* what) {
    std::vector<char> s(4096, 0x5a), before(s);
    const std::string err = wt::fill(t, "test", d.data(), d.size(), s.data());
    char where[64];
    snprintf(where, sizeof where, "weights[%d] (%s)", idx, idx >= 0 ? t[idx].name : "");
    const bool ok = !err.empty() && (idx < 0 || err.find(where) != std::string::npos) &&
                    err.find(what) != std::string::npos;
    if (!ok) printf("expected a refusal naming %s and '%s', got: '%s'\n", idx < 0 ? "the list" : where, what, err.c_str());
    CHECK(ok);
    CHECK(s == before);
}

int main() {
    const wt::Table &vit = wt::vit_table(false, 530), &vits = wt::vit_table(true, 1370);
    const wt::Table &loftr = wt::loftr_table(0), &loftr_t = wt::loftr_table(123456);
    CHECK(&wt::vit_table(false, 530) == &vit && &wt::loftr_table(0) == &loftr);  // built once per parameter value
    // the three hub networks over wt::DinoFlat: ViT-S split and plain, ViT-B, ViT-L
    const wt::Table &dss = wt::dino_table(true, 530, 384, 12), &dsp = wt::dino_table(false, 530, 384, 12),
                    &dbs = wt::dino_table(true, 530, 768, 12), &dls = wt::dino_table(true, 530, 1024, 24);
    CHECK(&wt::dino_table(true, 530, 1024, 24) == &dls && &dss != &dsp);
    const wt::Table& crica = wt::crica_table();
    const wt::Table &salad = wt::salad_table(), &sp = wt::sp_table(), &lg = wt::lg_table(), &sg = wt::sg_table(),
                    &rn = wt::rn_table(), &mxt = wt::mixvpr_trunk_table(), &mxh = wt::mixvpr_head_table();

    // ---- lengths: the list lengths of the operators
    CHECK(vit.size() == 174 && vits.size() == 174);
    CHECK(dss.size() == 174 && dsp.size() == 174 && dbs.size() == 174 && wt::dino_table(false, 530, 768, 12).size() == 174);
    CHECK(dls.size() == 342 && wt::dino_table(false, 530, 1024, 24).size() == 342);  // 4 + 14 x 24 + 2
    CHECK(crica.size() == 24);
    CHECK(salad.size() == 8);
    CHECK(sp.size() == 24);
    CHECK(lg.size() == 234);  // 1 + 2 x 9 x 10 + 4 x 9 + 2 x 8 + 1
    CHECK(sg.size() == 156);
    CHECK(rn.size() == 130);
    CHECK(mxt.size() == 106 && mxh.size() == 7);
    CHECK(loftr.size() == 129 && loftr_t.size() == 130);

    // ---- tiling
    check_tiling("vit", {&vit}, sizeof(mlg_vit_weights), {HEAD, TAIL_FROM(mlg_vit_weights, packing)});
    check_tiling("vit split", {&vits}, sizeof(mlg_vit_weights), {HEAD, TAIL_FROM(mlg_vit_weights, packing)});
    {
        // DinoFlat: mlg_dino_weights, whose `blocks` pointer is set after the fill, then the block array
        using D = wt::DinoFlat;
        using W = mlg_dino_weights;
        static_assert(offsetof(D, w) == 0 && offsetof(D, blocks) == sizeof(W), "no padding between the two");
        const std::vector<Span> others{HEAD, Span{offsetof(W, embed), offsetof(W, patch_w) - offsetof(W, embed)},
                                       Span{offsetof(W, blocks), sizeof(void*)}, TAIL_FROM(W, packing)};
        std::vector<Span> others12 = others;  // depth 12 leaves the upper twelve blocks alone
        others12.push_back({offsetof(D, blocks) + 12 * sizeof(mlg_vit_block), 12 * sizeof(mlg_vit_block)});
        static_assert(MLG_DINO_MAX_DEPTH == 24, "the unused blocks above");
        check_tiling("dino ViT-S split", {&dss}, sizeof(D), others12);
        check_tiling("dino ViT-S", {&dsp}, sizeof(D), others12);
        check_tiling("dino ViT-B split", {&dbs}, sizeof(D), others12);
        check_tiling("dino ViT-L split", {&dls}, sizeof(D), others);
    }
    check_tiling("crica", {&crica}, sizeof(mlg_crica_weights),
                 {HEAD, Span{offsetof(mlg_crica_weights, gem_p),
                             offsetof(mlg_crica_weights, layers) - offsetof(mlg_crica_weights, gem_p)}});
    check_tiling("salad", {&salad}, sizeof(mlg_salad_weights), {HEAD, TAIL_FROM(mlg_salad_weights, dust_bin)});
    check_tiling("superpoint", {&sp}, sizeof(mlg_sp_weights), {HEAD});
    check_tiling("lightglue", {&lg}, sizeof(mlg_lg_weights), {HEAD});
    {
        // a SuperGlue layer has no LayerNorm: its list leaves ln_g / ln_b (adjacent) out
        std::vector<Span> others{HEAD, TAIL_FROM(mlg_sg_weights, bin_score)};
        static_assert(offsetof(mlg_lg_block, ln_b) == offsetof(mlg_lg_block, ln_g) + sizeof(void*), "adjacent");
        for (int i = 0; i < 18; ++i)
            others.push_back({offsetof(mlg_sg_weights, layer) + i * sizeof(mlg_lg_block) + offsetof(mlg_lg_block, ln_g),
                              2 * sizeof(void*)});
        check_tiling("superglue", {&sg}, sizeof(mlg_sg_weights), others);
    }
    check_tiling("resnet50", {&rn}, sizeof(mlg_rn_weights), {HEAD});
    check_tiling("mixvpr", {&mxt, &mxh}, sizeof(mlg_mixvpr_weights), {HEAD});
    check_tiling("loftr + tails", {&loftr_t}, sizeof(mlg_loftr_weights), {HEAD});
    check_tiling("loftr", {&loftr}, sizeof(mlg_loftr_weights),
                 {HEAD, Span{offsetof(mlg_loftr_weights, coarse_tails), sizeof(void*)}});

    // ---- element counts that depend on a parameter or a shared shape table
    CHECK(vit[find(vit, "pos")].numel == 530 * 768 && vits[find(vits, "pos")].numel == 1370 * 768);
    CHECK(vit[find(vit, "blocks[0].qkv_w")].numel == 2304 * 768 && vits[find(vits, "blocks[0].qkv_w")].numel == 2 * 2304 * 768);
    CHECK(vits[find(vits, "patch_w")].numel == 2 * 768 * 768 && vits[find(vits, "blocks[11].fc2_b")].numel == 768);
    // ViT-S split: GEMM weight rows padded to the split GEMM's 256-row tile, [W_hi | W_lo]; biases keep their count
    CHECK(dss[find(dss, "patch_w")].numel == 512 * 768 * 2 && dss[find(dss, "blocks[0].qkv_w")].numel == 1280 * 384 * 2);
    CHECK(dss[find(dss, "blocks[0].proj_w")].numel == 512 * 384 * 2 && dss[find(dss, "blocks[0].fc1_w")].numel == 1536 * 384 * 2);
    CHECK(dss[find(dss, "blocks[0].fc2_w")].numel == 512 * 1536 * 2 && dss[find(dss, "blocks[0].qkv_b")].numel == 1152);
    CHECK(dsp[find(dsp, "patch_w")].numel == 384 * 768 && dsp[find(dsp, "blocks[0].qkv_w")].numel == 1152 * 384);  // plain: none
    CHECK(crica[find(crica, "layers[1].fc2_w")].numel == 768 * 2 * 2048);
    // ViT-B's table is the general one at (768, 12): entry for entry the dino table, each field at its place
    // in mlg_dino_weights (net level) or in the block array
    for (const bool split : {false, true})
        for (const int64_t tokens : {530, 1370}) {
            const wt::Table &v = wt::vit_table(split, tokens), &d = wt::dino_table(split, tokens, 768, 12);
            CHECK(v.size() == d.size());
            const struct { const char* name; size_t off; } net[] = {
                {"patch_w", offsetof(mlg_dino_weights, patch_w)}, {"patch_b", offsetof(mlg_dino_weights, patch_b)},
                {"cls", offsetof(mlg_dino_weights, cls)},         {"pos", offsetof(mlg_dino_weights, pos)},
                {"norm_w", offsetof(mlg_dino_weights, norm_w)},   {"norm_b", offsetof(mlg_dino_weights, norm_b)}};
            size_t n_net = 0;
            for (size_t i = 0; i < v.size() && i < d.size(); ++i) {
                CHECK(!strcmp(v[i].name, d[i].name) && v[i].kind == d[i].kind && v[i].numel == d[i].numel &&
                      v[i].optional == d[i].optional);
                if (!strncmp(d[i].name, "blocks[", 7)) {
                    CHECK(d[i].offset - offsetof(wt::DinoFlat, blocks) == v[i].offset - offsetof(mlg_vit_weights, blocks));
                    continue;
                }
                for (const auto& f : net)
                    if (!strcmp(d[i].name, f.name)) {
                        CHECK(d[i].offset - offsetof(wt::DinoFlat, w) == f.off);
                        ++n_net;
                    }
            }
            CHECK(n_net == 6);
        }
    CHECK(sp[find(sp, "w[8]")].numel == 128 * 256 && sp[find(sp, "b[8]")].numel == 128);
    CHECK(sp[find(sp, "w[3]")].numel == 128 * 9 * 64);
    CHECK(rn[find(rn, "blocks[0].w1")].numel == 128 * 64 && rn[find(rn, "blocks[0].wd")].numel == 256 * 64);
    CHECK(rn[find(rn, "blocks[3].wd")].numel == 512 * 256 && rn[find(rn, "blocks[15].w3")].numel == 2048 * 512);
    CHECK(!rn[find(rn, "blocks[13].wd")].optional && rn[find(rn, "blocks[14].wd")].optional);
    CHECK(loftr[find(loftr, "conv_w[4]")].numel == 256 * 9 * 128 && loftr[find(loftr, "conv_b[20]")].numel == 128);
    CHECK(loftr[find(loftr, "fine[1].w1")].numel == 256 * 256 && loftr[find(loftr, "coarse[0].w")].numel == 768 * 256);
    CHECK(lg[find(lg, "cross[0].Wqkv")].numel == 512 * 256 && lg[find(lg, "self[0].Wqkv")].numel == 768 * 256);

    // ---- the filler writes tensor i at the field entry i names
    {
        const mlg_vit_weights s = filled<mlg_vit_weights>(vit);
        AT(vit, s, patch_w, "patch_w");
        AT(vit, s, pos, "pos");
        AT(vit, s, blocks[0].norm1_w, "blocks[0].norm1_w");
        AT(vit, s, blocks[0].ls2, "blocks[0].ls2");
        AT(vit, s, blocks[11].norm1_w, "blocks[11].norm1_w");
        AT(vit, s, blocks[11].fc1_w, "blocks[11].fc1_w");
        AT(vit, s, blocks[11].ls2, "blocks[11].ls2");
        AT(vit, s, norm_b, "norm_b");
        CHECK(s.patch_w == tag(0) && s.blocks[0].norm1_w == tag(4) && s.norm_b == tag(173));
    }
    {
        const wt::DinoFlat s = filled<wt::DinoFlat>(dls);
        AT(dls, s, w.patch_w, "patch_w");
        AT(dls, s, w.pos, "pos");
        AT(dls, s, blocks[0].norm1_w, "blocks[0].norm1_w");
        AT(dls, s, blocks[12].qkv_w, "blocks[12].qkv_w");
        AT(dls, s, blocks[23].ls2, "blocks[23].ls2");
        AT(dls, s, w.norm_w, "norm_w");
        CHECK(s.w.patch_w == tag(0) && s.blocks[23].ls2 == tag(339) && s.w.norm_b == tag(341));
        CHECK(s.w.blocks == nullptr && s.w.embed == 0 && s.w.packing == 0);  // the caller's: left alone
        const wt::DinoFlat s12 = filled<wt::DinoFlat>(dss);
        CHECK(s12.blocks[11].ls2 == tag(171) && s12.blocks[12].norm1_w == nullptr && s12.w.norm_b == tag(173));
    }
    {
        const mlg_crica_weights s = filled<mlg_crica_weights>(crica);
        AT(crica, s, layers[0].in_w, "layers[0].in_w");
        AT(crica, s, layers[0].ln2_b, "layers[0].ln2_b");
        AT(crica, s, layers[1].fc2_w, "layers[1].fc2_w");
        CHECK(s.layers[0].in_w == tag(0) && s.layers[1].in_w == tag(12) && s.layers[1].ln2_b == tag(23));
    }
    {
        const mlg_salad_weights s = filled<mlg_salad_weights>(salad);
        AT(salad, s, w1, "w1");
        AT(salad, s, b2, "b2");
        AT(salad, s, bt2, "bt2");
        CHECK(s.w1 == tag(0) && s.bt2 == tag(7));
    }
    {
        const mlg_sp_weights s = filled<mlg_sp_weights>(sp);
        AT(sp, s, conv1a_w, "conv1a_w");
        AT(sp, s, conv1a_b, "conv1a_b");
        AT(sp, s, w[0], "w[0]");
        AT(sp, s, w[10], "w[10]");
        AT(sp, s, b[0], "b[0]");
        AT(sp, s, b[10], "b[10]");
        CHECK(s.w[0] == tag(2) && s.b[0] == tag(13) && s.b[10] == tag(23));
    }
    {
        const mlg_lg_weights s = filled<mlg_lg_weights>(lg);
        AT(lg, s, Wr, "Wr");
        AT(lg, s, self[0].Wqkv, "self[0].Wqkv");
        AT(lg, s, self[3].Wf1, "self[3].Wf1");
        AT(lg, s, self[8].bf2, "self[8].bf2");
        AT(lg, s, cross[0].Wqkv, "cross[0].Wqkv");
        AT(lg, s, cross[8].ln_b, "cross[8].ln_b");
        AT(lg, s, cross[8].bf2, "cross[8].bf2");
        AT(lg, s, Wfinal[0], "Wfinal[0]");
        AT(lg, s, Wfinal[8], "Wfinal[8]");
        AT(lg, s, bmatch[8], "bmatch[8]");
        AT(lg, s, wconf[0], "wconf[0]");
        AT(lg, s, bconf[7], "bconf[7]");
        AT(lg, s, ones, "ones");
        CHECK(s.Wr == tag(0) && s.self[3].Wf1 == tag(35) && s.cross[0].Wqkv == tag(91) && s.ones == tag(233));
    }
    {
        const mlg_sg_weights s = filled<mlg_sg_weights>(sg);
        AT(sg, s, kenc_w[0], "kenc_w[0]");
        AT(sg, s, kenc_w[2], "kenc_w[2]");
        AT(sg, s, kenc_b[0], "kenc_b[0]");
        AT(sg, s, kenc_b5, "kenc_b5");
        AT(sg, s, layer[0].Wqkv, "layer[0].Wqkv");
        AT(sg, s, layer[0].Wf2, "layer[0].Wf2");
        AT(sg, s, layer[17].bf1, "layer[17].bf1");
        AT(sg, s, layer[17].bf2, "layer[17].bf2");
        AT(sg, s, bfinal, "bfinal");
        CHECK(s.layer[0].ln_g == nullptr && s.layer[17].ln_b == nullptr);  // not in the list: left alone
        CHECK(s.kenc_b[0] == tag(3) && s.layer[0].Wf2 == tag(16) && s.bfinal == tag(155));
    }
    {
        const mlg_rn_weights s = filled<mlg_rn_weights>(rn);
        AT(rn, s, stem_w, "stem_w");
        AT(rn, s, stem_b, "stem_b");
        AT(rn, s, blocks[0].w1, "blocks[0].w1");
        AT(rn, s, blocks[0].bd, "blocks[0].bd");
        AT(rn, s, blocks[7].w2, "blocks[7].w2");
        AT(rn, s, blocks[15].w1, "blocks[15].w1");
        AT(rn, s, blocks[15].bd, "blocks[15].bd");
        CHECK(s.blocks[0].w1 == tag(2) && s.blocks[15].bd == tag(129));
    }
    {
        mlg_mixvpr_weights s;
        memset(&s, 0, sizeof s);
        std::vector<wt::Desc> d = good(mxt);
        CHECK(wt::fill(mxt, "test", d.data(), d.size(), &s).empty());
        CHECK(s.mix_w == nullptr && s.row_b == nullptr);  // the trunk's table leaves the head alone
        d = good(mxh);
        for (wt::Desc& x : d) x.ptr = (const char*)x.ptr + 0x100000;
        CHECK(wt::fill(mxh, "test", d.data(), d.size(), &s).empty());
        AT(mxt, s, stem_w, "stem_w");
        AT(mxt, s, blocks[0].w1, "blocks[0].w1");
        AT(mxt, s, blocks[12].w1, "blocks[12].w1");
        AT(mxt, s, blocks[12].bd, "blocks[12].bd");
        CHECK((const char*)s.mix_w == (const char*)tag(0) + 0x100000);
        CHECK((const char*)s.chan_w == (const char*)tag(3) + 0x100000);
        CHECK((const char*)s.row_b == (const char*)tag(6) + 0x100000);
    }
    {
        const mlg_loftr_weights s = filled<mlg_loftr_weights>(loftr_t);
        AT(loftr_t, s, stem_w, "stem_w");
        AT(loftr_t, s, conv_w[0], "conv_w[0]");
        AT(loftr_t, s, conv_w[20], "conv_w[20]");
        AT(loftr_t, s, conv_b[0], "conv_b[0]");
        AT(loftr_t, s, conv_b[20], "conv_b[20]");
        AT(loftr_t, s, coarse[0].w, "coarse[0].w");
        AT(loftr_t, s, coarse[7].ln2_b, "coarse[7].ln2_b");
        AT(loftr_t, s, fine[0].w, "fine[0].w");
        AT(loftr_t, s, fine[1].ln2_b, "fine[1].ln2_b");
        AT(loftr_t, s, merge_b, "merge_b");
        AT(loftr_t, s, coarse_tails, "coarse_tails");
        CHECK(s.conv_w[0] == tag(2) && s.conv_b[0] == tag(23) && s.coarse[0].w == tag(44) && s.coarse_tails == tag(129));
        const mlg_loftr_weights s0 = filled<mlg_loftr_weights>(loftr);
        CHECK(s0.coarse_tails == nullptr && s0.merge_b == tag(128));
    }

    // ---- every rejection, with the slot's index and field name
    {
        const int i = find(lg, "self[3].Wf1"), j = find(lg, "self[3].bf1");
        std::vector<wt::Desc> d = good(lg);
        d[i].kind = wt::F32;
        refuse(lg, d, i, "got f32");
        d = good(lg);
        d[j].kind = wt::BF16;
        refuse(lg, d, j, "got bf16");
        d = good(lg);
        d[j].kind = wt::OTHER;
        refuse(lg, d, j, "got another dtype");
        d = good(lg);
        d[i].device = -1;
        refuse(lg, d, i, "got a host tensor");
        d = good(lg);
        d[i].device = 1;
        refuse(lg, d, i, "got a tensor on device 1");
        d = good(lg);
        for (wt::Desc& x : d) x.device = -1;  // a host list with one device tensor in it
        d[j].device = 0;
        refuse(lg, d, j, "got a tensor on device 0");
        d = good(lg);
        d[i].contiguous = false;
        refuse(lg, d, i, "got a non-contiguous view");
        d = good(lg);
        d[i].numel -= 1;
        refuse(lg, d, i, "got 262143 elements");
        d = good(lg);
        d[i].numel += 1;
        refuse(lg, d, i, "got 262145 elements");
        d = good(lg);
        d[i].ptr = (const char*)d[i].ptr + 2;
        refuse(lg, d, i, "not 16-byte aligned");
        d = good(lg);
        d[j].ptr = (const char*)d[j].ptr + 4;  // f32: 16-byte alignment is not asked of it
        {
            mlg_lg_weights s;
            CHECK(wt::fill(lg, "test", d.data(), d.size(), &s).empty());
        }
        d = good(lg);
        d[i].numel = 0;
        d[i].ptr = nullptr;
        refuse(lg, d, i, "got 0 elements");  // empty where not optional
        d = good(lg);
        d.pop_back();
        refuse(lg, d, -1, "expected 234 tensors, got 233");
        d = good(lg);
        d.push_back(d[0]);
        refuse(lg, d, -1, "expected 234 tensors, got 235");
        for (wt::Desc& x : d) x.device = -1;  // an all-host list is one device too
        d.pop_back();
        {
            mlg_lg_weights s;
            CHECK(wt::fill(lg, "test", d.data(), d.size(), &s).empty());
        }
    }
    {
        // the ViT-L table: a list one block short, and a wrong count in the last block
        static_assert(sizeof(wt::DinoFlat) <= 4096, "refuse() hands the filler 4096 bytes");
        std::vector<wt::Desc> d = good(dls);
        d.erase(d.begin() + 4 + 23 * 14, d.begin() + 4 + 24 * 14);
        refuse(dls, d, -1, "expected 342 tensors, got 328");
        const int i = find(dls, "blocks[23].fc2_w");
        CHECK(i == 4 + 23 * 14 + 11);
        d = good(dls);
        d[i].numel = 768 * 3072 * 2;  // ViT-B's
        refuse(dls, d, i, "with 8388608 elements, contiguous, on device 0 as weights[0]; got 4718592 elements");
    }
    {
        // ResNet's downsample slots: required in a stage's first block, empty = NULL elsewhere
        const int first = find(rn, "blocks[3].wd"), later = find(rn, "blocks[4].wd");
        std::vector<wt::Desc> d = good(rn);
        d[first] = {nullptr, wt::BF16, 0, 0, true};
        refuse(rn, d, first, "got 0 elements");
        d = good(rn);
        d[later] = {nullptr, wt::BF16, 0, 0, true};
        d[later + 1] = {nullptr, wt::BF16, 0, 0, true};  // an empty tensor's kind does not matter
        mlg_rn_weights s;
        memset(&s, 0xff, sizeof s);
        CHECK(wt::fill(rn, "test", d.data(), d.size(), &s).empty());
        CHECK(s.blocks[4].wd == nullptr && s.blocks[4].bd == nullptr && s.blocks[4].w3 == tag(later - 2));
        CHECK(s.blocks[3].wd == tag(first));  // a non-empty wd is taken as it is
        d = good(rn);
        d[later].numel -= 1;  // non-empty where optional: still the entry's count
        refuse(rn, d, later, "expected empty or bf16");
        d = good(rn);
        d[later] = {nullptr, wt::BF16, 0, -1, true};  // an empty tensor still has to share the device
        refuse(rn, d, later, "got a host tensor");
    }
    {
        // LoFTR: conv_b of the convs without BatchNorm, and the packed tails
        std::vector<wt::Desc> d = good(loftr_t);
        const int cb = find(loftr_t, "conv_b[14]"), tl = find(loftr_t, "coarse_tails");
        d[cb] = {nullptr, wt::F32, 0, 0, true};
        d[tl] = {nullptr, wt::U8, 0, 0, true};
        mlg_loftr_weights s;
        memset(&s, 0xff, sizeof s);
        CHECK(wt::fill(loftr_t, "test", d.data(), d.size(), &s).empty());
        CHECK(s.conv_b[14] == nullptr && s.coarse_tails == nullptr && s.conv_b[13] == tag(cb - 1));
        d = good(loftr_t);
        d[tl].numel -= 1;
        refuse(loftr_t, d, tl, "got 123455 elements");
        d = good(loftr_t);
        d[tl].kind = wt::F32;
        refuse(loftr_t, d, tl, "expected empty or u8");
        const int cw = find(loftr_t, "conv_w[14]");
        d = good(loftr_t);
        d[cw] = {nullptr, wt::BF16, 0, 0, true};
        refuse(loftr_t, d, cw, "got 0 elements");
    }

    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
