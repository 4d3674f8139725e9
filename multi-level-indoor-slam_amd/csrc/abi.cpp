// Public C ABI (include/mlgate.h): DINOv2 ViT forward orchestration, kNN gate,
// op-level entry points and HIP-event profiling.
#include <hip/hip_runtime.h>

#include <math.h>

#include <mutex>
#include <vector>

#include "../../include/mlgate.h"
#include <cstddef>

#include "common.h"
#include "kernels.h"
#include "ws_carve.h"

namespace {

constexpr int PATCH = 14;

// E: the token width of the network (384 ViT-S, 768 ViT-B, 1024 ViT-L); heads of 64, MLP 4 E
struct VitGeom {
    int B, S, grid, P, T, Tpad, E, heads;
    explicit VitGeom(int b, int s, int e = MLG_VIT_EMBED)
        : B(b), S(s), grid(s / PATCH), P(grid * grid), T(grid * grid + 1), E(e), heads(e / 64) {
        Tpad = (T + 63) / 64 * 64;
    }
};

// depth of the hub network of width E, 0: no such network
int dino_depth(int E) { return E == 384 || E == 768 ? 12 : E == 1024 ? 24 : 0; }

// The trunk's view of a weight struct (mlg_vit_weights: 12 blocks inline; mlg_dino_weights: a
// host array of `depth`)
struct VitNet {
    const uint16_t* patch_w;
    const float *patch_b, *cls, *pos;
    const mlg_vit_block* blocks;
    int depth;
    const float *norm_w, *norm_b;
};
VitNet net_of(const mlg_vit_weights* w) {
    return {w->patch_w, w->patch_b, w->cls, w->pos, w->blocks, MLG_VIT_DEPTH, w->norm_w, w->norm_b};
}
VitNet net_of(const mlg_dino_weights* w) {
    return {w->patch_w, w->patch_b, w->cls, w->pos, w->blocks, w->depth, w->norm_w, w->norm_b};
}

// Operand buffers are sized for the split-bf16 forward (MLG_VIT_SPLIT): [hi | lo] rows
// for patches / xn / o / h, and q / k / vt as a hi plane followed by a lo plane (lo_elems
// apart); the plain bf16 forward uses the first half of each.
struct VitWorkspace {
    bf16_t *patches, *xn, *q, *k, *vt, *o, *h;
    float *x, *partial;
    int32_t* tasks;  // attention tasks + output offsets, 5 * B int32
    size_t q_bytes, vt_bytes, lo_elems;
};

// the ViT buffers at the carver's position (AnyLoc carves its own behind them)
VitWorkspace vit_take(WsCarver& c, const VitGeom& g) {
    const size_t rows = (size_t)g.B * g.T;
    const size_t heads = (size_t)g.B * g.heads, E = g.E;
    VitWorkspace w{};
    w.patches = c.take<bf16_t>((size_t)g.B * g.P * MLG_VIT_PATCH_K * 2);
    w.x = c.take<float>(rows * E);
    w.xn = c.take<bf16_t>(rows * E * 2);
    w.lo_elems = heads * g.Tpad * 64;
    w.q_bytes = w.vt_bytes = 2 * w.lo_elems * sizeof(bf16_t);
    w.q = c.take<bf16_t>(2 * w.lo_elems);
    w.k = c.take<bf16_t>(2 * w.lo_elems);
    w.vt = c.take<bf16_t>(2 * w.lo_elems);
    w.o = c.take<bf16_t>(rows * E * 2);
    w.h = c.take<bf16_t>(rows * 4 * E * 2);
    w.partial = c.take<float>(mlg_gem_partial_bytes(g.B, g.E) / sizeof(float));
    w.tasks = c.take<int32_t>((size_t)g.B * 5);
    return w;
}

size_t carve(const VitGeom& g, void* base, VitWorkspace* ws) {
    WsCarver c(base);
    const VitWorkspace w = vit_take(c, g);
    if (ws) *ws = w;
    return c.total();
}

// AnyLoc: the ViT buffers, then the patch tokens, the mean-pooled rows the final norm kernel
// also writes (unused), then the VLAD head's workspace
struct AnylocBufs {
    VitWorkspace vit;
    float *tokens, *pooled;  // [B, T - 2, 768]; [B, 768]
    char* head;
    size_t head_bytes;
};

// 0 when the VLAD head refuses (B, T - 2, K)
size_t anyloc_carve(const VitGeom& g, int K, void* base, AnylocBufs* out) {
    WsCarver c(base);
    AnylocBufs b;
    b.vit = vit_take(c, g);
    b.tokens = c.take<float>((size_t)g.B * (g.T - 2) * 768);
    b.pooled = c.take<float>((size_t)g.B * 768);
    b.head_bytes = mlg_vlad_ws_bytes(g.B, g.T - 2, K);
    b.head = c.take<char>(b.head_bytes);
    if (out) *out = b;
    return b.head_bytes ? c.total() : 0;
}

// CricaVPR's head inside the ViT workspace: the pooled rows, and the GeM descriptor the final
// norm kernel also writes (unused), in `h`, dead after the last block; the encoder's buffers
// in `x`, dead once the pyramid and the final norm have read it
struct CricaBufs {
    VitWorkspace vit;
    float *pooled, *gem;  // [B, 14, 768]; [B, 768]
    void* head;
    size_t head_bytes;
};

// 0 when the head does not fit the dead trunk buffers (never at image_size >= 168)
size_t crica_carve(const VitGeom& g, void* base, CricaBufs* out) {
    const size_t rows = (size_t)g.B * g.T;
    WsCarver c(base);
    CricaBufs b;
    b.vit = vit_take(c, g);
    WsCarver in_h(b.vit.h);
    b.pooled = in_h.take<float>((size_t)g.B * MLG_CRICA_ROWS * 768);
    b.gem = in_h.take<float>((size_t)g.B * 768);
    b.head = b.vit.x;
    b.head_bytes = mlg_crica_head_ws_bytes(g.B);
    if (out) *out = b;
    const bool fits = b.head_bytes && in_h.total() <= rows * 3072 * 2 * sizeof(bf16_t) &&
                      b.head_bytes <= rows * 768 * sizeof(float);
    return fits ? c.total() : 0;
}

// k <= 32 and D % 4 == 0 take the fused scan (no [Q, N] matrix): normalised rows plus
// the per-split partial lists
bool knn_fused(int D, int k) { return k >= 1 && k <= 32 && D % 4 == 0; }

struct KnnBufs {
    float *Xn, *Qn, *S;
    char* part;  // the fused scan's partial lists
};

// fused layouts: gate = Xn | partial lists; query = Xn | Qn | partial lists; else Xn | Qn | S
size_t knn_carve(int N, int D, int Q, int k, int query, void* base, KnnBufs* out) {
    WsCarver c(base);
    KnnBufs b{};
    b.Xn = c.take<float>((size_t)N * D);
    if (knn_fused(D, k)) {
        if (query) b.Qn = c.take<float>((size_t)Q * D);
        b.part = c.take<char>(mlg_knn_fused_ws_bytes(Q, N, k));
    } else {
        b.Qn = c.take<float>((size_t)Q * D);  // a gap on the gate path (its queries are rows of Xn): the size stays
        b.S = c.take<float>((size_t)Q * N);
    }
    if (out) *out = b;
    return c.total();
}

struct XcorrBufs {
    float *qn, *mn, *C;
};

size_t xcorr_carve(int n1, int n2, int D, void* base, XcorrBufs* out) {
    WsCarver c(base);
    XcorrBufs b;
    b.qn = c.take<float>((size_t)n1 * D);
    b.mn = c.take<float>((size_t)n2 * D);
    b.C = c.take<float>((size_t)n1 * n2);
    if (out) *out = b;
    return c.total();
}

// ------------------------------------------------------------- profiling
struct Prof {
    std::mutex mu;
    unsigned mask = 0;  // slots being recorded
    std::vector<hipEvent_t> pool;
    struct Rec { int slot; hipEvent_t a, b; double work; };
    std::vector<Rec> recs;
    size_t next = 0;
    double total[MLG_PROF_SLOTS] = {0};
    double work[MLG_PROF_SLOTS] = {0};
    long count[MLG_PROF_SLOTS] = {0};
} g_prof;

constexpr size_t PROF_POOL = 32768;

void prof_collect() {
    for (auto& r : g_prof.recs) {
        float ms = 0.f;
        (void)hipEventSynchronize(r.b);
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            g_prof.total[r.slot] += ms;
            g_prof.work[r.slot] += r.work;
            g_prof.count[r.slot] += 1;
        }
    }
    g_prof.recs.clear();
    g_prof.next = 0;
}

}  // namespace

MlgProfScope::MlgProfScope(int slot_, hipStream_t s_, double work_) : slot(slot_), s(s_), work(work_) {
    if (slot < 0 || slot >= MLG_PROF_SLOTS || !(g_prof.mask & (1u << slot))) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.next + 2 > g_prof.pool.size()) return;  // pool exhausted: stop recording
    a = g_prof.pool[g_prof.next++];
    b = g_prof.pool[g_prof.next++];
    (void)hipEventRecord(a, s);
}

MlgProfScope::~MlgProfScope() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.recs.push_back({slot, a, b, work});
}

extern "C" {

int mlg_abi_version(void) { return MLG_ABI_VERSION; }

const char* mlg_strerror(int status) {
    switch (status) {
        case MLG_OK: return "ok";
        case MLG_EINVAL: return "invalid argument (shape, alignment or size)";
        case MLG_EHIP: return "HIP launch error";
        case MLG_ENOMEM: return "workspace too small";
        case MLG_ESIZE: return "image size differs from the batch size";
        case MLG_EUNSUP: return "valid stream outside the supported subset";
        default: return "unknown mlgate status";
    }
}

size_t mlg_vit_workspace_bytes(int batch, int image_size) {
    if (batch <= 0 || image_size <= 0 || image_size % PATCH) return 0;
    return carve(VitGeom(batch, image_size), nullptr, nullptr);
}

}  // extern "C"

// Preprocess + patch embedding + the blocks; leaves the residual stream in ws->x.
// flags: MLG_VIT_KEEP_CHANNELS, and MLG_VIT_SPLIT for the split forward (weights packed
// [W_hi | W_lo], 2x the reduction dimension); each step picks its split or plain launcher.
static int vit_trunk(const VitNet& w, const uint8_t* frames, const VitGeom& g, int H, int W, int C,
                     long frame_stride, int flags, const VitWorkspace& ws, hipStream_t s) {
    const int M = g.B * g.T, E = g.E, F = 4 * g.E;
    const int swap_rb = (flags & MLG_VIT_KEEP_CHANNELS) ? 0 : 1, split = (flags & MLG_VIT_SPLIT) ? 1 : 0;
    MLG_TRY(mlg_preprocess_patches(frames, g.B, H, W, C, frame_stride, g.S, MLG_VIT_PATCH_K, swap_rb, ws.patches, s,
                                   split));
    MLG_TRY((split ? mlg_gemm_patch_split : mlg_gemm_patch)(ws.patches, w.patch_w, w.patch_b, w.pos, ws.x, g.B * g.P,
                                                            g.P, MLG_VIT_PATCH_K, s, E));
    MLG_TRY(mlg_cls_rows(ws.x, w.cls, w.pos, g.B, g.T, s, E));
    // padded key columns of V^T must be finite (masked keys multiply them by p = 0); padded
    // query rows are never stored but are zeroed too, so no lane computes on stale bits
    if (hipMemsetAsync(ws.vt, 0, ws.vt_bytes, s) != hipSuccess) return MLG_EHIP;
    if (hipMemsetAsync(ws.q, 0, ws.q_bytes, s) != hipSuccess) return MLG_EHIP;

    const double mul = split ? 3.0 : 1.0;  // MFMA products per algorithmic product
    const auto ln = [&](const float* gamma, const float* beta) {
        return (split ? mlg_layernorm_split : mlg_layernorm_bf16)(ws.x, gamma, beta, ws.xn, M, s, E);
    };
    // x += ls * (a W^T + b), a [M, K]: the projection (slot 3) and fc2 (slot 1)
    const auto residual = [&](int slot, const bf16_t* a, const bf16_t* wt, const float* b, const float* ls, int K) {
        MlgProfScope p(slot, s, mul * 2.0 * M * (double)E * K);
        return (split ? mlg_gemm_residual_split : mlg_gemm_residual)(a, wt, b, ls, ws.x, M, E, K, s);
    };
    for (int l = 0; l < w.depth; ++l) {
        const mlg_vit_block& bl = w.blocks[l];
        MLG_TRY(ln(bl.norm1_w, bl.norm1_b));
        {
            MlgProfScope p(2, s, mul * 2.0 * M * (3.0 * E) * E);
            MLG_TRY(split ? mlg_gemm_qkv_split(ws.xn, bl.qkv_w, bl.qkv_b, ws.q, ws.k, ws.vt, M, g.T, g.Tpad, ws.lo_elems,
                                               s, E)
                          : mlg_gemm_qkv(ws.xn, bl.qkv_w, bl.qkv_b, ws.q, ws.k, ws.vt, M, g.T, g.Tpad, s, E));
        }
        {
            MlgProfScope p(4, s, mul * 4.0 * g.B * g.heads * (double)g.T * g.T * 64);
            MLG_TRY(split ? mlg_attention_split(ws.q, ws.k, ws.vt, ws.o, g.B, g.T, g.Tpad, ws.lo_elems, ws.tasks, s,
                                                g.heads)
                          : mlg_attention(ws.q, ws.k, ws.vt, ws.o, g.B, g.T, g.Tpad, ws.tasks, s, g.heads));
        }
        MLG_TRY(residual(3, ws.o, bl.proj_w, bl.proj_b, bl.ls1, E));
        MLG_TRY(ln(bl.norm2_w, bl.norm2_b));
        {
            MlgProfScope p(0, s, mul * 2.0 * M * (double)F * E);
            MLG_TRY((split ? mlg_gemm_bias_gelu_split : mlg_gemm_bias_gelu_bf16)(ws.xn, bl.fc1_w, bl.fc1_b, ws.h, M, F, E,
                                                                                  s));
        }
        MLG_TRY(residual(1, ws.h, bl.fc2_w, bl.fc2_b, bl.ls2, F));
    }
    return MLG_OK;
}

// What mlg_vit_forward and mlg_dino_forward share once their struct is checked
static int vit_forward_run(const VitNet& net, int packing, const VitGeom& g, const uint8_t* frames, int H, int W,
                           int C, long frame_stride, int flags, void* workspace, size_t workspace_bytes,
                           float* desc_out, float* local_out, void* stream) {
    // the split forward reads 2x-wide weight rows: plain weights with the flag would be read out of bounds
    if (packing != ((flags & MLG_VIT_SPLIT) ? MLG_VIT_SPLIT : 0)) return MLG_EINVAL;
    VitWorkspace ws;
    if (carve(g, workspace, &ws) > workspace_bytes) return MLG_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    const int mean_pool = (flags & MLG_VIT_POOL_MEAN) ? 1 : 0;
    MLG_TRY(vit_trunk(net, frames, g, H, W, C, frame_stride, flags, ws, s));
    MLG_TRY(mlg_final_norm_gem(ws.x, net.norm_w, net.norm_b, local_out, ws.partial, desc_out, g.B, g.T, mean_pool, s,
                               g.E));
    return MLG_OK;
}

extern "C" {

int mlg_vit_forward(const mlg_vit_weights* w, const uint8_t* frames, int batch, int H, int W, int C,
                    long frame_stride, int image_size, int flags, void* workspace, size_t workspace_bytes,
                    float* desc_out, float* local_out, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !frames || !workspace || !desc_out || batch <= 0 || image_size % PATCH)
        return MLG_EINVAL;
    return vit_forward_run(net_of(w), w->packing, VitGeom(batch, image_size), frames, H, W, C, frame_stride, flags,
                           workspace, workspace_bytes, desc_out, local_out, stream);
}

size_t mlg_dino_workspace_bytes(int embed, int batch, int image_size) {
    if (!dino_depth(embed) || batch <= 0 || image_size <= 0 || image_size % PATCH) return 0;
    return carve(VitGeom(batch, image_size, embed), nullptr, nullptr);
}

int mlg_dino_forward(const mlg_dino_weights* w, const uint8_t* frames, int batch, int H, int W, int C,
                     long frame_stride, int image_size, int flags, void* workspace, size_t workspace_bytes,
                     float* desc_out, float* local_out, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !frames || !workspace || !desc_out || batch <= 0 || image_size <= 0 ||
        image_size % PATCH)
        return MLG_EINVAL;
    // one of the three hub networks: width, its depth, heads of 64
    if (!dino_depth(w->embed) || w->depth != dino_depth(w->embed) || w->heads * 64 != w->embed || !w->blocks)
        return MLG_EINVAL;
    return vit_forward_run(net_of(w), w->packing, VitGeom(batch, image_size, w->embed), frames, H, W, C, frame_stride,
                           flags, workspace, workspace_bytes, desc_out, local_out, stream);
}

size_t mlg_salad_workspace_bytes(int batch, int image_size) {
    // the head reuses the ViT buffers: hidden [B*T, 1024] bf16 in `h`, scores / cluster
    // features [B*T, 256] f32 in `x` once the final LayerNorm has read it
    return mlg_vit_workspace_bytes(batch, image_size);
}

int mlg_salad_forward(const mlg_vit_weights* w, const mlg_salad_weights* sw, const uint8_t* frames, int batch,
                      int H, int W, int C, long frame_stride, int image_size, void* workspace,
                      size_t workspace_bytes, float* desc_out, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !mlg_head_ok(sw, MLG_ABI_VERSION) || !frames || !workspace || !desc_out ||
        batch <= 0 || image_size % PATCH)
        return MLG_EINVAL;
    if (w->packing != 0) return MLG_EINVAL;  // SALAD's trunk runs the plain bf16 forward
    const VitGeom g(batch, image_size);
    VitWorkspace ws;
    if (carve(g, workspace, &ws) > workspace_bytes) return MLG_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    const int M = g.B * g.T;
    // SALAD._preprocess keeps the stored channel order (place_recognition.py:395-397)
    MLG_TRY(vit_trunk(net_of(w), frames, g, H, W, C, frame_stride, MLG_VIT_KEEP_CHANNELS, ws, s));
    MLG_TRY(mlg_layernorm_bf16(ws.x, w->norm_w, w->norm_b, ws.xn, M, s));  // backbone norm_layer, all tokens
    MLG_TRY(mlg_gemm_bias_relu_bf16(ws.xn, 768, sw->w1, sw->b1, ws.h, 1024, 1024, M, 1024, 768, s));
    float* y = ws.x;  // [M, 256]
    MLG_TRY(mlg_gemm_bias_f32_ld(ws.h, 1024, sw->w2, sw->b2, y, 256, M, 256, 1024, s));
    MLG_TRY(mlg_salad_head(ws.xn, y, g.B, g.T, sw->wt1, sw->bt1, sw->wt2, sw->bt2, sw->dust_bin, desc_out, s));
    return MLG_OK;
}

size_t mlg_vlad_workspace_bytes(int B, int P, int K) { return mlg_vlad_ws_bytes(B, P, K); }

int mlg_op_vlad(const mlg_vlad_vocab* vocab, const float* tokens, int B, int P, void* workspace,
                size_t workspace_bytes, float* desc, int32_t* labels_or_null, void* stream) {
    if (!mlg_head_ok(vocab, MLG_ABI_VERSION)) return MLG_EINVAL;
    return mlg_vlad_run(vocab->centers, vocab->num_clusters, tokens, B, P, workspace, workspace_bytes, desc,
                        labels_or_null, (hipStream_t)stream);
}

size_t mlg_anyloc_workspace_bytes(int B, int image_size, int K) {
    if (!mlg_vit_workspace_bytes(B, image_size) || image_size < 2 * PATCH) return 0;
    return anyloc_carve(VitGeom(B, image_size), K, nullptr, nullptr);
}

int mlg_anyloc_forward(const mlg_vit_weights* w, const mlg_vlad_vocab* vocab, const uint8_t* frames, int B, int H,
                       int W, int C, long frame_stride, int image_size, int flags, void* workspace,
                       size_t workspace_bytes, float* desc, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !mlg_head_ok(vocab, MLG_ABI_VERSION) || !frames || !workspace || !desc)
        return MLG_EINVAL;
    if (w->packing != ((flags & MLG_VIT_SPLIT) ? MLG_VIT_SPLIT : 0)) return MLG_EINVAL;
    if (!mlg_anyloc_workspace_bytes(B, image_size, vocab->num_clusters)) return MLG_EINVAL;
    const VitGeom g(B, image_size);
    AnylocBufs b;
    if (anyloc_carve(g, vocab->num_clusters, workspace, &b) > workspace_bytes) return MLG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MLG_TRY(vit_trunk(net_of(w), frames, g, H, W, C, frame_stride, flags, b.vit, s));
    MLG_TRY(mlg_final_norm_gem(b.vit.x, w->norm_w, w->norm_b, b.tokens, b.vit.partial, b.pooled, g.B, g.T,
                               /*mean_pool=*/1, s));
    return mlg_vlad_run(vocab->centers, vocab->num_clusters, b.tokens, B, g.T - 2, b.head, b.head_bytes, desc, nullptr,
                        s);
}

size_t mlg_kmeans_workspace_bytes(long M, int K) { return mlg_kmeans_ws_bytes(M, K); }

int mlg_kmeans_step(const float* tokens, long M, float* centers, int K, int32_t* labels, int64_t* changed,
                    int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return mlg_kmeans_step_run(tokens, M, centers, K, labels, changed, counts, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

static int crica_trunk_args_ok(const mlg_vit_weights* w, const uint8_t* frames, int B, int image_size, int flags,
                               const void* workspace) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !frames || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return 0;
    if (B < 1 || B > MLG_CRICA_MAX_BATCH || image_size <= 0 || image_size % PATCH) return 0;
    return (flags & MLG_VIT_SPLIT) && w->packing == MLG_VIT_SPLIT;
}

int mlg_crica_forward(const mlg_vit_weights* w, const mlg_crica_weights* cw, const uint8_t* frames, int B, int H,
                      int W, int C, long frame_stride, int image_size, int flags, int group, void* workspace,
                      size_t workspace_bytes, float* desc_out, float* local_out_or_null, void* stream) {
    if (!mlg_head_ok(cw, MLG_ABI_VERSION) || !crica_trunk_args_ok(w, frames, B, image_size, flags, workspace))
        return MLG_EINVAL;
    if (!mlg_crica_weights_ok(*cw) || group < 1 || group > MLG_CRICA_MAX_GROUP) return MLG_EINVAL;
    if (!desc_out || ((reinterpret_cast<uintptr_t>(desc_out) | reinterpret_cast<uintptr_t>(local_out_or_null)) & 15))
        return MLG_EINVAL;
    if (image_size < MLG_CRICA_MIN_GRID * PATCH) return MLG_EINVAL;
    const VitGeom g(B, image_size);
    CricaBufs b;
    const size_t need = crica_carve(g, workspace, &b);
    if (!need) return MLG_EINVAL;
    if (need > workspace_bytes) return MLG_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    MLG_TRY(vit_trunk(net_of(w), frames, g, H, W, C, frame_stride, flags, b.vit, s));  // MLG_VIT_SPLIT: checked above
    MLG_TRY(mlg_crica_pool_run(b.vit.x, w->norm_w, w->norm_b, g.B, g.grid, cw->gem_p, b.pooled, s));
    if (local_out_or_null)  // the rerank cache: mlg_vit_forward's local features from this forward
        MLG_TRY(mlg_final_norm_gem(b.vit.x, w->norm_w, w->norm_b, local_out_or_null, b.vit.partial, b.gem, g.B, g.T,
                                   /*mean_pool=*/0, s));
    return mlg_crica_encoder_run(*cw, b.pooled, g.B, group, b.head, b.head_bytes, desc_out, s);
}

int mlg_op_vit_trunk(const mlg_vit_weights* w, const uint8_t* frames, int B, int H, int W, int C, long frame_stride,
                     int image_size, int flags, void* workspace, size_t workspace_bytes, float* tokens_prenorm,
                     void* stream) {
    if (!crica_trunk_args_ok(w, frames, B, image_size, flags, workspace) || !tokens_prenorm) return MLG_EINVAL;
    const VitGeom g(B, image_size);
    VitWorkspace ws;
    if (carve(g, workspace, &ws) > workspace_bytes) return MLG_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    MLG_TRY(vit_trunk(net_of(w), frames, g, H, W, C, frame_stride, flags, ws, s));  // MLG_VIT_SPLIT: checked above
    if (hipMemcpyAsync(tokens_prenorm, ws.x, (size_t)g.B * g.T * 768 * sizeof(float), hipMemcpyDeviceToDevice, s) !=
        hipSuccess)
        return MLG_EHIP;
    return MLG_OK;
}

int mlg_op_crica_pool(const float* tokens_prenorm, const float* norm_w, const float* norm_b, int B, int grid,
                      float gem_p, float* out, void* stream) {
    return mlg_crica_pool_run(tokens_prenorm, norm_w, norm_b, B, grid, gem_p, out, (hipStream_t)stream);
}

int mlg_op_crica_encoder(const mlg_crica_weights* cw, const float* pooled, int B, int group, void* workspace,
                         size_t workspace_bytes, float* desc, void* stream) {
    if (!mlg_head_ok(cw, MLG_ABI_VERSION)) return MLG_EINVAL;
    return mlg_crica_encoder_run(*cw, pooled, B, group, workspace, workspace_bytes, desc, (hipStream_t)stream);
}

size_t mlg_knn_workspace_bytes(int N, int D, int Q) {
    if (N <= 0 || D <= 0 || Q <= 0) return 0;
    return knn_carve(N, D, Q, /*k=*/0, 0, nullptr, nullptr);  // k = 0: never fused
}

size_t mlg_knn_workspace_bytes_k(int N, int D, int Q, int k, int query) {
    if (N <= 0 || D <= 0 || Q <= 0) return 0;
    return knn_carve(N, D, Q, k, query, nullptr, nullptr);
}

int mlg_knn_gate(const float* desc, int N, int D, const double* t, const int64_t* floor, const uint8_t* has_floor,
                 double min_gap, float thr, int k, int gating, int q0, int Q, void* workspace,
                 size_t workspace_bytes, int32_t* idx, float* sim, uint8_t* valid, int32_t* count,
                 unsigned long long* totals, void* stream) {
    if (!desc || !t || !workspace || N <= 0 || D <= 0 || Q <= 0 || q0 < 0 || q0 + Q > N) return MLG_EINVAL;
    if (gating && (!floor || !has_floor)) return MLG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    KnnBufs b;
    if (knn_carve(N, D, Q, k, 0, workspace, &b) > workspace_bytes) return MLG_ENOMEM;
    if (knn_fused(D, k)) {
        MLG_TRY(mlg_row_normalize_wave(desc, b.Xn, N, D, nullptr, s));
        return mlg_knn_fused(b.Xn + (size_t)q0 * D, Q, b.Xn, N, D, t + q0, t, gating ? floor + q0 : nullptr,
                             gating ? has_floor + q0 : nullptr, gating ? floor : nullptr, gating ? has_floor : nullptr,
                             min_gap, thr, k, gating, b.part, idx, sim, valid, count, totals, s);
    }
    MLG_TRY(mlg_row_normalize(desc, b.Xn, N, D, nullptr, s));
    MLG_TRY(mlg_similarity_f32(b.Xn + (size_t)q0 * D, Q, b.Xn, N, D, b.S, N, s));
    MLG_TRY(mlg_topk_gate(b.S, N, N, Q, t + q0, t, gating ? floor + q0 : nullptr, gating ? has_floor + q0 : nullptr,
                          gating ? floor : nullptr, gating ? has_floor : nullptr, min_gap, thr, k, gating, idx, sim,
                          valid, count, totals, s));
    return MLG_OK;
}

int mlg_knn_query(const float* db, int N, int D, const float* qdesc, int Q, const double* t_db,
                  const double* t_query, double min_gap, int k, void* workspace, size_t workspace_bytes,
                  int32_t* idx, float* sim, int32_t* count, void* stream) {
    if (!db || !qdesc || !t_db || !t_query || !workspace || N <= 0 || D <= 0 || Q <= 0) return MLG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    KnnBufs b;
    if (knn_carve(N, D, Q, k, 1, workspace, &b) > workspace_bytes) return MLG_ENOMEM;
    if (knn_fused(D, k)) {
        MLG_TRY(mlg_row_normalize_wave(db, b.Xn, N, D, nullptr, s));
        MLG_TRY(mlg_row_normalize_wave(qdesc, b.Qn, Q, D, nullptr, s));
        return mlg_knn_fused(b.Qn, Q, b.Xn, N, D, t_query, t_db, nullptr, nullptr, nullptr, nullptr, min_gap,
                             -INFINITY, k, 0, b.part, idx, sim, nullptr, count, nullptr, s);
    }
    MLG_TRY(mlg_row_normalize(db, b.Xn, N, D, nullptr, s));
    MLG_TRY(mlg_row_normalize(qdesc, b.Qn, Q, D, nullptr, s));
    MLG_TRY(mlg_similarity_f32(b.Qn, Q, b.Xn, N, D, b.S, N, s));
    MLG_TRY(mlg_topk_gate(b.S, N, N, Q, t_query, t_db, nullptr, nullptr, nullptr, nullptr, min_gap, -INFINITY, k, 0,
                          idx, sim, nullptr, count, nullptr, s));
    return MLG_OK;
}

size_t mlg_knn_append_workspace_bytes(int n_old, int n_new, int D, int k) {
    if (n_old < 0 || n_new <= n_old || !knn_fused(D, k)) return 0;
    return mlg_knn_append_ws_bytes(n_old, n_new, k);
}

int mlg_knn_append(const float* xn, int n_old, int n_new, int D, const double* t, const int64_t* floor,
                   const uint8_t* has_floor, double min_gap, float thr, int k, int gating, void* workspace,
                   size_t workspace_bytes, int32_t* idx, float* sim, uint8_t* valid, int32_t* count,
                   int32_t* inserted, int32_t* evicted_idx, int32_t* n_evicted, void* stream) {
    return mlg_op_knn_append_phases(xn, n_old, n_new, D, t, floor, has_floor, min_gap, thr, k, gating, workspace,
                                    workspace_bytes, idx, sim, valid, count, inserted, evicted_idx, n_evicted,
                                    MLG_KNN_APPEND_UPDATE | MLG_KNN_APPEND_FRESH, stream);
}

int mlg_op_knn_append_phases(const float* xn, int n_old, int n_new, int D, const double* t, const int64_t* floor,
                             const uint8_t* has_floor, double min_gap, float thr, int k, int gating, void* workspace,
                             size_t workspace_bytes, int32_t* idx, float* sim, uint8_t* valid, int32_t* count,
                             int32_t* inserted, int32_t* evicted_idx, int32_t* n_evicted, int phases, void* stream) {
    if (phases < 1 || phases > (MLG_KNN_APPEND_UPDATE | MLG_KNN_APPEND_FRESH)) return MLG_EINVAL;
    if (n_old < 0 || n_new <= n_old || D <= 0 || !knn_fused(D, k)) return MLG_EINVAL;
    if (!xn || !t || !workspace || !idx || !sim || !valid || !count) return MLG_EINVAL;
    if (n_old > 0 && (!inserted || !evicted_idx || !n_evicted)) return MLG_EINVAL;
    if (gating && (!floor || !has_floor)) return MLG_EINVAL;
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (misaligned(xn, 16) || misaligned(t, 8) || misaligned(floor, 8) || misaligned(workspace, 16) ||
        misaligned(idx, 4) || misaligned(sim, 4) || misaligned(count, 4) || misaligned(inserted, 4) ||
        misaligned(evicted_idx, 4) || misaligned(n_evicted, 4))
        return MLG_EINVAL;
    return mlg_knn_append_run(xn, n_old, n_new, D, t, floor, has_floor, min_gap, thr, k, gating, workspace,
                              workspace_bytes, idx, sim, valid, count, inserted, evicted_idx, n_evicted,
                              (hipStream_t)stream, phases);
}

int mlg_row_normalize_f32(const float* X, float* Xn, int N, int D, float* norms_or_null, void* stream) {
    return mlg_row_normalize(X, Xn, N, D, norms_or_null, (hipStream_t)stream);
}

int mlg_similarity(const float* A, int Q, const float* B, int N, int D, float* S, void* stream) {
    return mlg_similarity_f32(A, Q, B, N, D, S, N, (hipStream_t)stream);
}

size_t mlg_plane_ransac_workspace_bytes(int S, int iterations) { return mlg_plane_ws_bytes(S, iterations); }

int mlg_plane_ransac(const float* pts, const int32_t* offsets, int S, int iterations, uint64_t seed, double threshold,
                     void* workspace, size_t workspace_bytes, double* plane, double* ratio, int32_t* inliers,
                     void* stream) {
    if (!pts || !offsets || !workspace || !plane || !ratio || !inliers) return MLG_EINVAL;
    return mlg_plane_ransac_run(pts, offsets, S, iterations, seed, threshold, workspace, workspace_bytes, plane,
                                ratio, inliers, (hipStream_t)stream);
}

size_t mlg_proximity_workspace_bytes(int N, int nrows) { return mlg_proximity_ws_bytes(N, nrows); }

int mlg_proximity_count(const double* pos, const int64_t* floor, int N, int row0, int nrows, double radius,
                        int min_gap, int strict, void* workspace, size_t workspace_bytes, long long* totals,
                        void* stream) {
    if ((!pos && N > 0) || !workspace || !totals) return MLG_EINVAL;
    return mlg_proximity_count_run(pos, floor, N, row0, nrows, radius, min_gap, strict, workspace, workspace_bytes,
                                   totals, (hipStream_t)stream);
}

int mlg_proximity_emit(const double* pos, const int64_t* floor, int N, int row0, int nrows, double radius,
                       int min_gap, int strict, const void* workspace, size_t workspace_bytes, int32_t* pairs,
                       double* dist, uint8_t* valid, void* stream) {
    if ((!pos && N > 0) || !workspace || !pairs || !dist || !valid) return MLG_EINVAL;
    return mlg_proximity_emit_run(pos, floor, N, row0, nrows, radius, min_gap, strict, workspace, workspace_bytes,
                                  pairs, dist, valid, (hipStream_t)stream);
}

size_t mlg_resnet50_workspace_bytes(int B, int H, int W) { return mlg_resnet50_ws_bytes(B, H, W); }

int mlg_resnet50_forward(const mlg_rn_weights* w, const uint8_t* frames, int B, int H, int W, int C,
                         long frame_stride, int descriptor_dim, void* workspace, size_t workspace_bytes,
                         float* desc, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !frames || !workspace || !desc || !w->stem_w || !w->stem_b)
        return MLG_EINVAL;
    for (int i = 0; i < 16; ++i) {
        const mlg_rn_block& b = w->blocks[i];
        if (!b.w1 || !b.b1 || !b.w2 || !b.b2 || !b.w3 || !b.b3) return MLG_EINVAL;
        const bool first = i == 0 || i == 3 || i == 7 || i == 13;
        if (first != (b.wd != nullptr) || (b.wd && !b.bd)) return MLG_EINVAL;
    }
    if (frame_stride < (long)H * W * C) return MLG_EINVAL;
    return mlg_resnet50_run(*w, frames, B, H, W, C, frame_stride, descriptor_dim, workspace, workspace_bytes, desc,
                            nullptr, (hipStream_t)stream);
}

int mlg_op_pillow_resize_224(const uint8_t* frames, int B, int H, int W, int C, long frame_stride, void* workspace,
                             size_t workspace_bytes, uint8_t* out, void* stream) {
    if (!frames || !workspace || !out || frame_stride < (long)H * W * C) return MLG_EINVAL;
    const mlg_rn_weights none{};  // the resize reads no weights
    return mlg_resnet50_run(none, frames, B, H, W, C, frame_stride, 1, workspace, workspace_bytes, nullptr, out,
                            (hipStream_t)stream);
}

size_t mlg_mixvpr_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return mlg_resnet50_l3_ws_bytes(B, MLG_MIXVPR_SIZE);
}

static bool mixvpr_head_ok(const mlg_mixvpr_weights* w) {
    return w->mix_w && w->mix_p && w->row_w && w->chan_w && w->chan_b && w->row_s && w->row_b;
}

int mlg_mixvpr_forward(const mlg_mixvpr_weights* w, const uint8_t* frames, int B, int H, int W, int C,
                       long frame_stride, void* workspace, size_t workspace_bytes, float* desc, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !frames || !workspace || !desc || !w->stem_w || !w->stem_b ||
        !mixvpr_head_ok(w))
        return MLG_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || frame_stride < (long)H * W * C)
        return MLG_EINVAL;
    for (int i = 0; i < 13; ++i) {
        const mlg_rn_block& b = w->blocks[i];
        if (!b.w1 || !b.b1 || !b.w2 || !b.b2 || !b.w3 || !b.b3) return MLG_EINVAL;
        const bool first = i == 0 || i == 3 || i == 7;
        if (first != (b.wd != nullptr) || (b.wd && !b.bd)) return MLG_EINVAL;
    }
    if (workspace_bytes < mlg_mixvpr_workspace_bytes(B, H, W)) return MLG_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    MLG_TRY(mlg_mixvpr_preprocess(frames, B, H, W, C, frame_stride,
                                  mlg_resnet50_l3_image(workspace, B, MLG_MIXVPR_SIZE), s));
    float* feat = nullptr;
    MLG_TRY(mlg_resnet50_l3_run(w->stem_w, w->stem_b, w->blocks, B, MLG_MIXVPR_SIZE, workspace, workspace_bytes, &feat,
                                s));
    return mlg_mixvpr_head(*w, feat, B, desc, s);
}

int mlg_op_mixvpr_preprocess(const uint8_t* frames, int B, int H, int W, int C, long frame_stride, float* out,
                             void* stream) {
    return mlg_mixvpr_preprocess(frames, B, H, W, C, frame_stride, out, (hipStream_t)stream);
}

int mlg_op_mixvpr_head(const mlg_mixvpr_weights* w, const float* features, int B, float* desc, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !mixvpr_head_ok(w)) return MLG_EINVAL;
    return mlg_mixvpr_head(*w, features, B, desc, (hipStream_t)stream);
}

size_t mlg_superpoint_workspace_bytes(int B, int H, int W) { return mlg_superpoint_ws_bytes(B, H, W); }

int mlg_superpoint(const mlg_sp_weights* w, const uint8_t* frames, int B, int H, int W, int C, long frame_stride,
                   float detection_threshold, int max_keypoints, int nms_radius, int remove_borders, void* workspace,
                   size_t workspace_bytes, float* keypoints, float* scores, float* descriptors,
                   uint16_t* descriptors_bf16, int32_t* counts, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !frames || !workspace || !keypoints || !scores || !descriptors || !counts)
        return MLG_EINVAL;
    if (!w->conv1a_w || !w->conv1a_b) return MLG_EINVAL;
    for (int i = 0; i < 11; ++i) {
        if (!w->w[i] || !w->b[i]) return MLG_EINVAL;
        if ((reinterpret_cast<uintptr_t>(w->w[i]) & 15) || (reinterpret_cast<uintptr_t>(w->b[i]) & 15))
            return MLG_EINVAL;
    }
    if (frame_stride < (long)H * W * C) return MLG_EINVAL;
    return mlg_superpoint_run(*w, frames, B, H, W, C, frame_stride, detection_threshold, max_keypoints, nms_radius,
                              remove_borders, workspace, workspace_bytes, keypoints, scores, descriptors,
                              descriptors_bf16, counts, (hipStream_t)stream);
}

size_t mlg_lightglue_workspace_bytes(int P, int kmax) { return mlg_lightglue_ws_bytes(P, kmax); }

int mlg_lightglue(const mlg_lg_weights* w, const float* keypoints, const float* descriptors, const int32_t* counts,
                  int F, int kmax, const int32_t* pair_a, const int32_t* pair_b, int P, float depth_confidence,
                  float width_confidence, float filter_threshold, int pruning_min_kpts, void* workspace,
                  size_t workspace_bytes, int32_t* matches, float* scores, int32_t* num_matches, int32_t* stop_layer,
                  void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !keypoints || !descriptors || !counts || !pair_a || !pair_b || !workspace ||
        !matches || !scores || !num_matches || F <= 0 || P <= 0)
        return MLG_EINVAL;
    for (int p = 0; p < P; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= F || pair_b[p] < 0 || pair_b[p] >= F) return MLG_EINVAL;
    return mlg_lightglue_run(*w, keypoints, descriptors, counts, kmax, pair_a, pair_b, P, depth_confidence,
                             width_confidence, filter_threshold, pruning_min_kpts, workspace, workspace_bytes,
                             matches, scores, num_matches, stop_layer, (hipStream_t)stream);
}

size_t mlg_superglue_workspace_bytes(int P, int kmax) { return mlg_superglue_ws_bytes(P, kmax); }

int mlg_superglue(const mlg_sg_weights* w, const float* keypoints, const float* scores, const float* descriptors,
                  const int32_t* counts, int F, int kmax, int W, int H, const int32_t* pair_a, const int32_t* pair_b,
                  int P, int sinkhorn_iterations, float match_threshold, void* workspace, size_t workspace_bytes,
                  int32_t* matches, float* match_scores, int32_t* num_matches, void* stream) {
    if (!mlg_head_ok(w, MLG_ABI_VERSION) || !keypoints || !scores || !descriptors || !counts || !pair_a || !pair_b ||
        !workspace || !matches || !match_scores || !num_matches || F <= 0 || P <= 0 || W <= 0 || H <= 0)
        return MLG_EINVAL;
    for (int p = 0; p < P; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= F || pair_b[p] < 0 || pair_b[p] >= F) return MLG_EINVAL;
    return mlg_superglue_run(*w, keypoints, scores, descriptors, counts, kmax, W, H, pair_a, pair_b, P,
                             sinkhorn_iterations, match_threshold, workspace, workspace_bytes, matches, match_scores,
                             num_matches, (hipStream_t)stream);
}

size_t mlg_ransac_workspace_bytes(int P, long S_total, int hypotheses) {
    return mlg_ransac_ws_bytes(P, S_total, hypotheses);
}

int mlg_ransac_epipolar(const float* kp1, const float* kp2, const int32_t* offsets, int P, long S_total,
                        const double* K, int k_stride, double threshold, int hypotheses, uint64_t seed,
                        void* workspace, size_t workspace_bytes, double* model, uint8_t* mask, int32_t* inliers,
                        double* pose, int32_t* status, void* stream) {
    if (!offsets || !workspace || !model || !inliers || !status || (S_total > 0 && (!kp1 || !kp2 || !mask)))
        return MLG_EINVAL;
    if (K && k_stride != 0 && k_stride != 9) return MLG_EINVAL;
    return mlg_ransac_run(kp1, kp2, offsets, P, S_total, K, k_stride, threshold, hypotheses, seed, workspace,
                          workspace_bytes, model, mask, inliers, pose, status, (hipStream_t)stream);
}

int mlg_recover_pose(const float* kp1, const float* kp2, const int32_t* offsets, int P, const double* K,
                     int k_stride, const double* E, const uint8_t* mask, double* pose, void* stream) {
    if (!kp1 || !kp2 || !offsets || !K || !E || !mask || !pose) return MLG_EINVAL;
    if (k_stride != 0 && k_stride != 9) return MLG_EINVAL;
    return mlg_recover_pose_run(kp1, kp2, offsets, P, K, k_stride, E, mask, pose, (hipStream_t)stream);
}

size_t mlg_xcorr_workspace_bytes(int n1, int n2, int D) {
    if (n1 <= 0 || n2 <= 0 || D <= 0) return 0;
    return xcorr_carve(n1, n2, D, nullptr, nullptr);
}

int mlg_xcorr_score(const float* q, int n1, const float* m, int n2, int D, void* workspace, size_t workspace_bytes,
                    float* score, void* stream) {
    if (!q || !m || !workspace || !score || n1 <= 0 || n2 <= 0 || D <= 0) return MLG_EINVAL;
    XcorrBufs b;
    if (xcorr_carve(n1, n2, D, workspace, &b) > workspace_bytes) return MLG_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    MLG_TRY(mlg_row_normalize(q, b.qn, n1, D, nullptr, s));
    MLG_TRY(mlg_row_normalize(m, b.mn, n2, D, nullptr, s));
    MLG_TRY(mlg_similarity_f32(b.qn, n1, b.mn, n2, D, b.C, n2, s));
    MLG_TRY(mlg_xcorr_reduce(b.C, n1, n2, score, s));
    return MLG_OK;
}

size_t mlg_xcorr_batch_workspace_bytes(int F, int L, int D, int P) { return mlg_xcorr_batch_ws_bytes(F, L, D, P); }

int mlg_xcorr_batch(const float* feats, int F, int L, int D, const int32_t* query, const int32_t* cand, int P,
                    void* workspace, size_t workspace_bytes, float* scores, void* stream) {
    return mlg_xcorr_batch_run(feats, F, L, D, query, cand, P, workspace, workspace_bytes, scores,
                               (hipStream_t)stream);
}

size_t mlg_rerank_workspace_bytes(int F, int L, int D, int Q, int k) { return mlg_rerank_ws_bytes(F, L, D, Q, k); }

int mlg_rerank_gate(const float* feats, int F, int L, int D, int q0, int Q, int k, const int32_t* idx,
                    const float* sim, const uint8_t* mask_or_null, const int32_t* count,
                    const uint8_t* cached_or_null, int top_k, void* workspace, size_t workspace_bytes,
                    int32_t* r_idx, float* r_sim, float* r_cross, double* r_score, int32_t* r_count,
                    unsigned long long* dropped_total_or_null, void* stream) {
    return mlg_rerank_run(feats, F, L, D, q0, Q, k, idx, sim, mask_or_null, count, cached_or_null, top_k, workspace,
                          workspace_bytes, r_idx, r_sim, r_cross, r_score, r_count, dropped_total_or_null,
                          (hipStream_t)stream);
}

size_t mlg_seq_workspace_bytes(int N, int D, int Q, int k) { return mlg_seq_ws_bytes(N, D, Q, k); }

int mlg_seq_gate(const float* desc, int N, int D, const double* t, const int64_t* floor, const uint8_t* has_floor,
                 int q0, int Q, int k, const int32_t* idx, const float* sim, const uint8_t* mask_or_null,
                 const int32_t* count, int radius, double min_gap, int min_terms, double threshold, void* workspace,
                 size_t workspace_bytes, double* s_score, int8_t* s_dir, int32_t* s_terms, uint8_t* keep,
                 unsigned long long* rejected_total_or_null, void* stream) {
    return mlg_seq_run(desc, N, D, t, floor, has_floor, q0, Q, k, idx, sim, mask_or_null, count, radius, min_gap,
                       min_terms, threshold, workspace, workspace_bytes, s_score, s_dir, s_terms, keep,
                       rejected_total_or_null, (hipStream_t)stream);
}

int mlg_op_gemm_f32out(const uint16_t* A, const uint16_t* W, float* C, int M, int N, int K, void* stream) {
    return mlg_gemm_f32out(A, W, C, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_f32out_variant(int variant, const uint16_t* A, const uint16_t* W, float* C, int M, int N, int K,
                               void* stream) {
    return mlg_gemm_f32out_variant(variant, A, W, C, M, N, K, (hipStream_t)stream);
}
int mlg_set_gemm_variant(int variant) { return mlg_gemm_set_variant(variant); }
int mlg_op_gemm_bias_gelu(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, int M, int N,
                          int K, void* stream) {
    return mlg_gemm_bias_gelu_bf16(A, W, bias, C, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_residual(const uint16_t* A, const uint16_t* W, const float* bias, const float* gamma, float* X,
                         int M, int N, int K, void* stream) {
    return mlg_gemm_residual(A, W, bias, gamma, X, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_residual_split(const uint16_t* A, const uint16_t* W, const float* bias, const float* gamma, float* X,
                               int M, int N, int K0, void* stream) {
    return mlg_gemm_residual_split(A, W, bias, gamma, X, M, N, K0, (hipStream_t)stream);
}
int mlg_op_gemm_bias_gelu_split(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, int M, int N,
                                int K0, void* stream) {
    return mlg_gemm_bias_gelu_split(A, W, bias, C, M, N, K0, (hipStream_t)stream);
}
int mlg_op_layernorm_bf16(const float* X, const float* g, const float* b, uint16_t* Y, int M, void* stream) {
    return mlg_layernorm_bf16(X, g, b, Y, M, (hipStream_t)stream);
}
int mlg_op_attention(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, uint16_t* O, int B, int T, int Tpad,
                     int32_t* task_ws, void* stream) {
    return mlg_attention(Q, K, Vt, O, B, T, Tpad, task_ws, (hipStream_t)stream);
}
int mlg_op_attention_varlen(const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, uint16_t* O, int ldo, int Npad,
                            int heads, const int32_t* tasks, const int32_t* out_off, int ntasks, int max_q,
                            void* stream) {
    return mlg_attention_varlen(Q, K, Vt, O, ldo, Npad, heads, reinterpret_cast<const int4*>(tasks), out_off, ntasks,
                                max_q, (hipStream_t)stream);
}
int mlg_op_lg_ffn(const uint16_t* ctx, float* X, uint16_t* xcopy, int ldc, int M, const uint16_t* Wout,
                  const float* bout, const uint16_t* Wf1, const float* bf1, const float* ln_g, const float* ln_b,
                  const uint16_t* Wf2, const float* bf2, void* stream) {
    mlg_lg_block w{};
    w.Wout = Wout; w.bout = bout; w.Wf1 = Wf1; w.bf1 = bf1; w.ln_g = ln_g; w.ln_b = ln_b; w.Wf2 = Wf2; w.bf2 = bf2;
    return mlg_lg_ffn(ctx, X, xcopy, ldc, M, w, (hipStream_t)stream);
}
int mlg_op_lg_proj(int self_block, const uint16_t* xcopy, int ldx, const uint16_t* W, const float* bias,
                   const float* ecos, const float* esin, const uint8_t* live, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                   int Npad, void* stream) {
    (void)esin;  // the factors come interleaved in `ecos` (lg_fac4 layout, include/mlgate.h)
    return mlg_lg_proj(self_block != 0, xcopy, ldx, W, bias, ecos, live, Q, K, Vt, Npad, (hipStream_t)stream);
}
int mlg_op_conv2d_nhwc(const uint16_t* in, const uint16_t* zero16, int B, int H, int W, int C, int k, int s,
                       const uint16_t* Wt, const float* bias, float* out, int N, void* stream) {
    return mlg_conv_implicit(in, zero16, B, H, W, C, k, s, Wt, bias, nullptr, 0, out, N, nullptr, 0, 0, N, N,
                             (hipStream_t)stream);
}
int mlg_op_conv2d_nhwc_epi(const uint16_t* in, const uint16_t* zero16, int B, int H, int W, int C, int k, int s,
                           const uint16_t* Wt, const float* bias, const float* R, int ldr, float* out, int ldx,
                           uint16_t* out16, int ldc, int act, int act_cols, int N, void* stream) {
    return mlg_conv_implicit(in, zero16, B, H, W, C, k, s, Wt, bias, R, ldr, out, ldx, out16, ldc, act, act_cols, N,
                             (hipStream_t)stream);
}
int mlg_op_gemm_conv(const uint16_t* A, int lda, const uint16_t* W, const float* bias, const float* R, int ldr,
                     float* X, int ldx, uint16_t* C, int ldc, int act, int act_cols, int M, int N, int K, float vdiv,
                     void* stream) {
    return mlg_gemm_conv(A, lda, W, bias, R, ldr, X, ldx, C, ldc, act, act_cols, M, N, K, (hipStream_t)stream, vdiv);
}
int mlg_op_gemm_conv_upadd(const uint16_t* A, int lda, const uint16_t* W, const float* bias, const float* src, int h,
                           int w, uint16_t* C, int M, int N, int K, void* stream) {
    return mlg_gemm_conv_upadd(A, lda, W, bias, src, h, w, C, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_bias_relu(const uint16_t* A, int lda, const uint16_t* W, const float* bias, uint16_t* C, int ldc,
                          int nvalid, int M, int N, int K, void* stream) {
    return mlg_gemm_bias_relu_bf16(A, lda, W, bias, C, ldc, nvalid, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_bias_add_relu(const uint16_t* A, int lda, const uint16_t* W, const float* bias, const float* R,
                              float* X, int ldx, uint16_t* C, int M, int N, int K, void* stream) {
    return mlg_gemm_bias_add_relu(A, lda, W, bias, R, X, ldx, C, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_bias_f32_ld(const uint16_t* A, int lda, const uint16_t* W, const float* bias, float* C, int ldc, int M,
                            int N, int K, void* stream) {
    return mlg_gemm_bias_f32_ld(A, lda, W, bias, C, ldc, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_bias_split(const uint16_t* A, int lda, const uint16_t* W, const float* bias, uint16_t* H, uint16_t* L,
                           int M, int N, int K, void* stream) {
    return mlg_gemm_bias_split_bf16(A, lda, W, bias, H, L, M, N, K, (hipStream_t)stream);
}
int mlg_op_gemm_qkv(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* Q, uint16_t* K, uint16_t* Vt,
                    int M, int T, int Tpad, void* stream) {
    return mlg_gemm_qkv(A, W, bias, Q, K, Vt, M, T, Tpad, (hipStream_t)stream);
}
int mlg_op_gemm_patch(const uint16_t* A, const uint16_t* W, const float* bias, const float* pos, float* X, int M,
                      int P, int Kpad, void* stream) {
    return mlg_gemm_patch(A, W, bias, pos, X, M, P, Kpad, (hipStream_t)stream);
}
int mlg_op_gemm_sim_split_loftr(const uint16_t* A, const uint16_t* B, int M, int Npad, int K0, float* S, int lds,
                                int ncols, int nb, long pstride, void* stream) {
    return mlg_gemm_sim_split_loftr(A, B, M, Npad, K0, S, lds, ncols, (hipStream_t)stream, nb, pstride);
}
int mlg_op_lg_ffn_ex(const uint16_t* ctx, float* X, uint16_t* xcopy, int ldc, int M, const uint16_t* Wout,
                     const float* bout, const uint16_t* Wf1, const float* bf1, const float* ln_g, const float* ln_b,
                     const uint16_t* Wf2, const float* bf2, int relu, const int32_t* rowseg, const float* wc,
                     const float* bc, const float* wm, const float* bm, float thr, float width, float* lz,
                     uint8_t* flags, void* stream) {
    mlg_lg_block w{};
    w.Wout = Wout; w.bout = bout; w.Wf1 = Wf1; w.bf1 = bf1; w.ln_g = ln_g; w.ln_b = ln_b; w.Wf2 = Wf2; w.bf2 = bf2;
    const mlg_lg_conf_i cf{rowseg, wc, bc, wm, bm, thr, width, lz, flags};
    return mlg_lg_ffn(ctx, X, xcopy, ldc, M, w, (hipStream_t)stream, &cf, relu);
}
int mlg_op_preprocess_patches(const uint8_t* frames, int B, int H, int W, int C, long frame_stride, int S,
                              uint16_t* patches, void* stream) {
    return mlg_preprocess_patches(frames, B, H, W, C, frame_stride, S, MLG_VIT_PATCH_K, 1, patches,
                                  (hipStream_t)stream);
}

int mlg_prof_enable(int slot_mask) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (slot_mask && g_prof.pool.empty()) {
        g_prof.pool.resize(PROF_POOL);
        for (auto& e : g_prof.pool)
            if (hipEventCreate(&e) != hipSuccess) return MLG_EHIP;
    }
    g_prof.mask = (unsigned)slot_mask & ((1u << MLG_PROF_SLOTS) - 1);
    return MLG_OK;
}

int mlg_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    prof_collect();
    for (int i = 0; i < MLG_PROF_SLOTS; ++i) {
        g_prof.total[i] = 0;
        g_prof.work[i] = 0;
        g_prof.count[i] = 0;
    }
    return MLG_OK;
}

int mlg_prof_read(int slot, double* total_ms, long* launches) {
    if (slot < 0 || slot >= MLG_PROF_SLOTS || !total_ms || !launches) return MLG_EINVAL;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    prof_collect();
    *total_ms = g_prof.total[slot];
    *launches = g_prof.count[slot];
    return MLG_OK;
}

int mlg_prof_read_work(int slot, double* flops) {
    if (slot < 0 || slot >= MLG_PROF_SLOTS || !flops) return MLG_EINVAL;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    prof_collect();
    *flops = g_prof.work[slot];
    return MLG_OK;
}

}  // extern "C"
