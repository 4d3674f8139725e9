#include <cstdlib>
// PyTorch-ROCm custom operators over the mlgate C ABI (include/mlgate.h).
//
// TORCH_LIBRARY(mlgate, m) declares one operator per ABI entry point the Python
// drop-in uses (mlgate/*.py call torch.ops.mlgate.*); TORCH_LIBRARY_IMPL(mlgate, CUDA, m)
// binds them for HIP tensors (PyTorch-ROCm names its HIP dispatch key CUDA).  Each
// operator checks devices / dtypes / shapes, allocates its outputs and workspace from
// the caching allocator and launches on the current HIP stream of the tensors' device,
// so the ops compose with torch streams, events and hipGraph capture (the ABI itself
// never allocates or synchronises; LightGlue and the proximity emit read one small
// device result back by design -- see the header).  Weights arrive as flat tensor
// lists (mlgate/*.py build them once); weight_tables.h holds each list's order and checks
// every tensor of it before anything is launched.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mlgate.h"
#include "weight_tables.h"

namespace {

using at::Tensor;

void check_rc(int rc, const char* what) { TORCH_CHECK(rc == MLG_OK, what, " failed: ", mlg_strerror(rc)); }

void* stream_of(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void want(const Tensor& t, at::ScalarType ty, const char* name, bool device = true) {
    TORCH_CHECK(t.scalar_type() == ty, name, ": expected ", ty, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    if (device) {
        TORCH_CHECK(t.is_cuda(), name, " must be on the HIP device");
    } else {
        TORCH_CHECK(t.device().is_cpu(), name, " must be a host tensor");
    }
}

template <typename T>
const T* cp(const Tensor& t) {
    return t.defined() && t.numel() > 0 ? reinterpret_cast<const T*>(t.data_ptr()) : nullptr;
}
template <typename T>
T* mp(const Tensor& t) {
    return t.defined() && t.numel() > 0 ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

Tensor workspace(size_t bytes, const Tensor& like) {
    Tensor t = at::empty({(int64_t)std::max<size_t>(bytes, 1)}, like.options().dtype(at::kByte));
    // diagnostic (MLG_WS_POISON=1): every workspace starts as all-ones bytes (NaN in f32 /
    // bf16), so a kernel that reads workspace it never wrote shows up as changed results
    static const bool poison = [] {
        const char* v = getenv("MLG_WS_POISON");
        return v && atoi(v) != 0;
    }();
    if (poison) t.fill_(255);
    return t;
}

// ------------------------------------------------------------ frame batches
// frames uint8 [B, H, W, C], contiguous, on the device; stride: bytes from one frame to the next
struct Frames {
    const uint8_t* p;
    int64_t B;
    int H, W, C;
    long stride;
};
Frames frames_of(const Tensor& frames) {
    want(frames, at::kByte, "frames");
    TORCH_CHECK(frames.dim() == 4, "frames must be [B, H, W, C]");
    const int64_t H = frames.size(1), W = frames.size(2), C = frames.size(3);
    return {cp<uint8_t>(frames), frames.size(0), (int)H, (int)W, (int)C, (long)(H * W * C)};
}

// call(b0, nb), an ABI call `what` on frames [b0, b0 + nb), for each run of at most `step` of B frames
template <class Call>
void for_chunks(int64_t B, int64_t step, const char* what, Call call) {
    for (int64_t b0 = 0; b0 < B; b0 += step) check_rc(call(b0, (int)std::min(step, B - b0)), what);
}

// ------------------------------------------------------------ weight lists
// Fill the pointer fields of *strukt from the list through its table (weight_tables.h).
// dev: the device the op launches on (the list must live there); none: any one device.
void fill_weights(const wt::Table& table, const char* model, at::TensorList w, void* strukt,
                  c10::optional<c10::Device> dev) {
    std::vector<wt::Desc> d;
    d.reserve(w.size());
    for (const Tensor& t : w) {
        TORCH_CHECK(t.defined(), model, " weights: undefined tensor");
        const at::ScalarType ty = t.scalar_type();
        const wt::Kind kind = ty == at::kBFloat16 ? wt::BF16
                              : ty == at::kFloat  ? wt::F32
                              : ty == at::kByte   ? wt::U8
                                                  : wt::OTHER;
        d.push_back({t.numel() ? t.data_ptr() : nullptr, kind, t.numel(),
                     t.device().is_cpu() ? -1 : (int)t.device().index(), t.is_contiguous()});
    }
    const std::string err = wt::fill(table, model, d.data(), d.size(), strukt);
    TORCH_CHECK(err.empty(), err);
    TORCH_CHECK(!dev.has_value() || (!w.empty() && w[0].device() == *dev), model, " weights must be on ", *dev);
}

// tokens of a ViT list of width `embed`, from the list's own `pos` (the ops take it from image_size)
int64_t tokens_of(at::TensorList w, int64_t embed) { return w.size() > 3 && w[3].defined() ? w[3].numel() / embed : 0; }

// ------------------------------------------------------------------ ViT-B/14
// split: weights packed for MLG_VIT_SPLIT ([W_hi | W_lo], 2x the reduction dim)
mlg_vit_weights vit_weights(at::TensorList w, bool split, int64_t image_size, c10::Device dev) {
    mlg_vit_weights s = MLG_STRUCT_INIT(mlg_vit_weights);
    const int64_t grid = image_size / 14;
    fill_weights(wt::vit_table(split, 1 + grid * grid), "vit", w, &s, dev);
    s.packing = split ? MLG_VIT_SPLIT : 0;
    return s;
}

// What vit_forward_into and dino_forward_into share once their weight struct is filled: desc
// f32 [B, embed] and local f32 [B, n_local, embed] (or none) are checked and written in calls
// of at most max_batch frames.  ws_bytes(nb): the workspace of nb frames; forward(frames, nb,
// ws, desc, local): the ABI call on one chunk.
template <class WsBytes, class Forward>
void forward_into(const Tensor& frames, const Frames& f, int64_t embed, int64_t image_size, int64_t max_batch,
                  const Tensor& desc, const c10::optional<Tensor>& local, const char* what, WsBytes ws_bytes,
                  Forward forward) {
    want(desc, at::kFloat, "desc");
    TORCH_CHECK(desc.dim() == 2 && desc.size(0) == f.B && desc.size(1) == embed, "desc must be [B, ", embed, "]");
    const int64_t grid = image_size / 14, n_local = grid * grid - 1;
    const bool has_local = local.has_value() && local->defined();
    if (has_local) {
        want(*local, at::kFloat, "local");
        TORCH_CHECK(local->dim() == 3 && local->size(0) == f.B && local->size(1) == n_local &&
                        local->size(2) == embed, "local must be [B, (S/14)^2 - 1, ", embed, "]");
    }
    TORCH_CHECK(max_batch > 0, "max_batch must be positive");
    c10::DeviceGuard g(frames.device());
    const Tensor ws = workspace(ws_bytes((int)std::min(f.B, max_batch)), frames);
    for_chunks(f.B, max_batch, what, [&](int64_t b0, int nb) {
        return forward(f.p + b0 * f.stride, nb, ws, mp<float>(desc) + b0 * embed,
                       has_local ? mp<float>(*local) + b0 * n_local * embed : nullptr);
    });
}

// frames uint8 [B, H, W, C]; writes desc f32 [B, 768] and local f32 [B, n_local, 768]
void vit_forward_into(const Tensor& frames, at::TensorList w, int64_t image_size, int64_t flags, int64_t max_batch,
                      const Tensor& desc, const c10::optional<Tensor>& local) {
    const Frames f = frames_of(frames);
    const mlg_vit_weights s = vit_weights(w, (flags & MLG_VIT_SPLIT) != 0, image_size, frames.device());
    forward_into(
        frames, f, MLG_VIT_EMBED, image_size, max_batch, desc, local, "mlg_vit_forward",
        [&](int nb) { return mlg_vit_workspace_bytes(nb, (int)image_size); },
        [&](const uint8_t* fr, int nb, const Tensor& ws, float* d, float* lo) {
            return mlg_vit_forward(&s, fr, nb, f.H, f.W, f.C, f.stride, (int)image_size, (int)flags, ws.data_ptr(),
                                   (size_t)ws.numel(), d, lo, stream_of(frames));
        });
}

// ------------------------------------------------------- DINOv2 ViT-S / B / L-14
// depth of the hub network of width `embed`; refuses any other width
int64_t dino_depth(int64_t embed) {
    TORCH_CHECK(embed == 384 || embed == 768 || embed == 1024, "dino: embed must be 384 (dinov2_vits14), 768 "
                "(dinov2_vitb14) or 1024 (dinov2_vitl14), got ", embed);
    return embed == 1024 ? 24 : 12;
}

void dino_weights(wt::DinoFlat& f, at::TensorList w, bool split, int64_t tokens, int64_t embed,
                  c10::optional<c10::Device> dev) {
    f.w = MLG_STRUCT_INIT(mlg_dino_weights);
    f.w.embed = (int)embed;
    f.w.depth = (int)dino_depth(embed);
    f.w.heads = (int)embed / 64;
    fill_weights(wt::dino_table(split, tokens, embed, f.w.depth), "dino", w, &f, dev);
    f.w.blocks = f.blocks;
    f.w.packing = split ? MLG_VIT_SPLIT : 0;
}

// vit_forward_into for the network of width `embed`: desc f32 [B, embed], local f32
// [B, n_local, embed]
void dino_forward_into(const Tensor& frames, at::TensorList w, int64_t embed, int64_t image_size, int64_t flags,
                       int64_t max_batch, const Tensor& desc, const c10::optional<Tensor>& local) {
    const Frames f = frames_of(frames);
    const int64_t grid = image_size / 14;
    wt::DinoFlat d;
    dino_weights(d, w, (flags & MLG_VIT_SPLIT) != 0, 1 + grid * grid, embed, frames.device());
    forward_into(
        frames, f, embed, image_size, max_batch, desc, local, "mlg_dino_forward",
        [&](int nb) { return mlg_dino_workspace_bytes((int)embed, nb, (int)image_size); },
        [&](const uint8_t* fr, int nb, const Tensor& ws, float* out, float* lo) {
            return mlg_dino_forward(&d.w, fr, nb, f.H, f.W, f.C, f.stride, (int)image_size, (int)flags, ws.data_ptr(),
                                    (size_t)ws.numel(), out, lo, stream_of(frames));
        });
}

// weights_check for a dino list (any one device, host included)
void dino_weights_check(at::TensorList w, int64_t embed, bool split) {
    dino_depth(embed);
    wt::DinoFlat f;
    dino_weights(f, w, split, tokens_of(w, embed), embed, c10::nullopt);
}

// SALAD: frames uint8 [B, H, W, C] -> desc f32 [B, 8448]
Tensor salad_forward(const Tensor& frames, at::TensorList w, at::TensorList salad, double dust_bin,
                     int64_t image_size, int64_t max_batch) {
    const Frames f = frames_of(frames);
    TORCH_CHECK(max_batch > 0, "max_batch must be positive");
    const mlg_vit_weights s = vit_weights(w, false, image_size, frames.device());
    mlg_salad_weights sw = MLG_STRUCT_INIT(mlg_salad_weights);
    fill_weights(wt::salad_table(), "salad", salad, &sw, frames.device());
    sw.dust_bin = (float)dust_bin;
    c10::DeviceGuard g(frames.device());
    Tensor desc = at::empty({f.B, MLG_SALAD_DIM}, frames.options().dtype(at::kFloat));
    Tensor ws = workspace(mlg_salad_workspace_bytes((int)std::min(f.B, max_batch), (int)image_size), frames);
    for_chunks(f.B, max_batch, "mlg_salad_forward", [&](int64_t b0, int nb) {
        return mlg_salad_forward(&s, &sw, f.p + b0 * f.stride, nb, f.H, f.W, f.C, f.stride, (int)image_size,
                                 ws.data_ptr(), (size_t)ws.numel(), mp<float>(desc) + b0 * MLG_SALAD_DIM,
                                 stream_of(frames));
    });
    return desc;
}

// --------------------------------------------------------------- retrieval
std::tuple<Tensor, Tensor, Tensor, Tensor> knn_gate(const Tensor& desc, const Tensor& t, const Tensor& floor,
                                                    const Tensor& has_floor, double min_gap, double thr, int64_t k,
                                                    bool gating, int64_t q0, int64_t Q,
                                                    const c10::optional<Tensor>& totals) {
    want(desc, at::kFloat, "desc");
    want(t, at::kDouble, "t");
    want(floor, at::kLong, "floor");
    want(has_floor, at::kByte, "has_floor");
    TORCH_CHECK(desc.dim() == 2, "desc must be [N, D]");
    const int64_t N = desc.size(0), D = desc.size(1);
    TORCH_CHECK(t.numel() == N && floor.numel() == N && has_floor.numel() == N, "t / floor / has_floor must be [N]");
    TORCH_CHECK(k >= 1, "k must be >= 1");
    TORCH_CHECK(q0 >= 0 && Q >= 0 && q0 + Q <= N, "query rows out of range");
    if (totals.has_value() && totals->defined()) {
        want(*totals, at::kLong, "totals");
        TORCH_CHECK(totals->numel() == 2, "totals must be int64 [2]");
    }
    c10::DeviceGuard g(desc.device());
    auto o = desc.options();
    Tensor idx = at::empty({Q, k}, o.dtype(at::kInt)), sim = at::empty({Q, k}, o.dtype(at::kFloat));
    Tensor valid = at::empty({Q, k}, o.dtype(at::kByte)), count = at::empty({Q}, o.dtype(at::kInt));
    Tensor ws = workspace(mlg_knn_workspace_bytes_k((int)N, (int)D, (int)Q, (int)k, 0), desc);
    check_rc(mlg_knn_gate(cp<float>(desc), (int)N, (int)D, cp<double>(t), cp<int64_t>(floor), cp<uint8_t>(has_floor),
                          min_gap, (float)thr, (int)k, gating ? 1 : 0, (int)q0, (int)Q, ws.data_ptr(),
                          (size_t)ws.numel(), mp<int32_t>(idx), mp<float>(sim), mp<uint8_t>(valid), mp<int32_t>(count),
                          (totals.has_value() && totals->defined()) ? mp<unsigned long long>(*totals) : nullptr,
                          stream_of(desc)),
             "mlg_knn_gate");
    return {idx, sim, valid, count};
}

std::tuple<Tensor, Tensor, Tensor> knn_query(const Tensor& db, const Tensor& q, const Tensor& t_db,
                                             const Tensor& t_q, double min_gap, int64_t k) {
    want(db, at::kFloat, "db");
    want(q, at::kFloat, "q");
    want(t_db, at::kDouble, "t_db");
    want(t_q, at::kDouble, "t_q");
    const int64_t N = db.size(0), D = db.size(1), Q = q.size(0);
    TORCH_CHECK(q.dim() == 2 && q.size(1) == D && t_db.numel() == N && t_q.numel() == Q, "knn_query shapes");
    TORCH_CHECK(k >= 1, "k must be >= 1");
    c10::DeviceGuard g(db.device());
    auto o = db.options();
    Tensor idx = at::empty({Q, k}, o.dtype(at::kInt)), sim = at::empty({Q, k}, o.dtype(at::kFloat));
    Tensor count = at::empty({Q}, o.dtype(at::kInt));
    Tensor ws = workspace(mlg_knn_workspace_bytes_k((int)N, (int)D, (int)Q, (int)k, 1), db);
    check_rc(mlg_knn_query(cp<float>(db), (int)N, (int)D, cp<float>(q), (int)Q, cp<double>(t_db), cp<double>(t_q),
                           min_gap, (int)k, ws.data_ptr(), (size_t)ws.numel(), mp<int32_t>(idx), mp<float>(sim),
                           mp<int32_t>(count), stream_of(db)),
             "mlg_knn_query");
    return {idx, sim, count};
}

Tensor row_normalize(const Tensor& X) {
    want(X, at::kFloat, "X");
    TORCH_CHECK(X.dim() == 2, "X must be [N, D]");
    c10::DeviceGuard g(X.device());
    Tensor Y = at::empty_like(X);
    check_rc(mlg_row_normalize_f32(cp<float>(X), mp<float>(Y), (int)X.size(0), (int)X.size(1), nullptr, stream_of(X)),
             "mlg_row_normalize_f32");
    return Y;
}

// S = A . B^T of row-normalised A [Q, D], B [N, D] (float32)
Tensor similarity(const Tensor& A, const Tensor& B) {
    want(A, at::kFloat, "A");
    want(B, at::kFloat, "B");
    TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(1) == B.size(1), "similarity shapes");
    c10::DeviceGuard g(A.device());
    Tensor S = at::empty({A.size(0), B.size(0)}, A.options());
    check_rc(mlg_similarity(cp<float>(A), (int)A.size(0), cp<float>(B), (int)B.size(0), (int)A.size(1), mp<float>(S),
                            stream_of(A)),
             "mlg_similarity");
    return S;
}

Tensor xcorr_score(const Tensor& q, const Tensor& m) {
    want(q, at::kFloat, "q");
    want(m, at::kFloat, "m");
    TORCH_CHECK(q.dim() == 2 && m.dim() == 2 && q.size(1) == m.size(1), "xcorr shapes");
    c10::DeviceGuard g(q.device());
    Tensor out = at::empty({1}, q.options());
    Tensor ws = workspace(mlg_xcorr_workspace_bytes((int)q.size(0), (int)m.size(0), (int)q.size(1)), q);
    check_rc(mlg_xcorr_score(cp<float>(q), (int)q.size(0), cp<float>(m), (int)m.size(0), (int)q.size(1), ws.data_ptr(),
                             (size_t)ws.numel(), mp<float>(out), stream_of(q)),
             "mlg_xcorr_score");
    return out;
}

// -------------------------------------------------------------- SuperPoint
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> superpoint(const Tensor& frames, at::TensorList w,
                                                               double det_thr, int64_t max_kp, int64_t nms_radius,
                                                               int64_t border, bool with_bf16) {
    want(frames, at::kByte, "frames");
    TORCH_CHECK(frames.dim() == 4, "frames must be [B, H, W, C]");
    mlg_sp_weights s = MLG_STRUCT_INIT(mlg_sp_weights);
    fill_weights(wt::sp_table(), "superpoint", w, &s, frames.device());
    const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2), C = frames.size(3);
    const size_t nbytes = mlg_superpoint_workspace_bytes((int)B, (int)H, (int)W);
    TORCH_CHECK(nbytes > 0, "SuperPoint needs H, W >= 16 (got ", H, "x", W, ")");
    c10::DeviceGuard g(frames.device());
    auto o = frames.options();
    Tensor kp = at::zeros({B, max_kp, 2}, o.dtype(at::kFloat)), sc = at::zeros({B, max_kp}, o.dtype(at::kFloat));
    Tensor ds = at::empty({B, max_kp, 256}, o.dtype(at::kFloat));
    Tensor db = with_bf16 ? at::empty({B, max_kp, 256}, o.dtype(at::kBFloat16)) : at::empty({0}, o.dtype(at::kBFloat16));
    Tensor cnt = at::empty({B}, o.dtype(at::kInt));
    Tensor ws = workspace(nbytes, frames);
    check_rc(mlg_superpoint(&s, cp<uint8_t>(frames), (int)B, (int)H, (int)W, (int)C, (long)(H * W * C), (float)det_thr,
                            (int)max_kp, (int)nms_radius, (int)border, ws.data_ptr(), (size_t)ws.numel(),
                            mp<float>(kp), mp<float>(sc), mp<float>(ds), with_bf16 ? mp<uint16_t>(db) : nullptr,
                            mp<int32_t>(cnt), stream_of(frames)),
             "mlg_superpoint");
    return {kp, sc, ds, db, cnt};
}

// ------------------------------------------------------------------ LoFTR
// the list with or without the packed coarse tails (loftr_pack_tails) at its end
constexpr size_t kLoftrTensors = 2 + 2 * MLG_LOFTR_NCONV + 10 * 8 + 5;

mlg_loftr_weights loftr_weights(at::TensorList w, c10::optional<c10::Device> dev) {
    mlg_loftr_weights s = MLG_STRUCT_INIT(mlg_loftr_weights);
    const int64_t tails = w.size() > kLoftrTensors ? (int64_t)mlg_loftr_tails_bytes() : 0;
    fill_weights(wt::loftr_table(tails), "loftr", w, &s, dev);
    return s;
}

// one coarse encoder layer in place, fused or unfused tail (mlg_op_loftr_coarse_layer)
void loftr_coarse_layer(const Tensor& x, const Tensor& cat, at::TensorList w, int64_t layer, int64_t fused,
                        int64_t nseg, int64_t L) {
    want(x, at::kFloat, "x");
    want(cat, at::kBFloat16, "cat");
    TORCH_CHECK(x.numel() == 2 * nseg * L * 256 && cat.numel() == 2 * nseg * L * 512,
                "x must be [2 nseg L, 256], cat [2 nseg L, 512]");
    const mlg_loftr_weights s = loftr_weights(w, x.device());
    c10::DeviceGuard g(x.device());
    Tensor ws = workspace(mlg_op_loftr_coarse_layer_ws_bytes((int)nseg, (int)L), x);
    check_rc(mlg_op_loftr_coarse_layer(&s, (int)layer, (int)fused, mp<float>(x), mp<uint16_t>(cat), (int)nseg, (int)L,
                                       ws.data_ptr(), (size_t)ws.numel(), stream_of(x)),
             "mlg_op_loftr_coarse_layer");
}

// the coarse block-tail weights packed once for the fused kernel (mlg_loftr_pack_tails)
Tensor loftr_pack_tails(at::TensorList w) {
    TORCH_CHECK(w.size() == kLoftrTensors, "loftr weights: expected ", kLoftrTensors, " tensors, got ", w.size());
    TORCH_CHECK(w[0].is_cuda(), "loftr weights must be on the HIP device");
    const mlg_loftr_weights s = loftr_weights(w, w[0].device());
    c10::DeviceGuard g(w[0].device());
    Tensor out = at::empty({(int64_t)mlg_loftr_tails_bytes()}, w[0].options().dtype(at::kByte));
    check_rc(mlg_loftr_pack_tails(&s, out.data_ptr(), stream_of(w[0])), "mlg_loftr_pack_tails");
    return out;
}

std::tuple<Tensor, Tensor> loftr_features(const Tensor& frames, at::TensorList w) {
    want(frames, at::kByte, "frames");
    TORCH_CHECK(frames.dim() == 4, "frames must be [B, H, W, C]");
    const mlg_loftr_weights s = loftr_weights(w, frames.device());
    const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2), C = frames.size(3);
    const size_t nbytes = mlg_loftr_features_ws_bytes((int)B, (int)H, (int)W);
    TORCH_CHECK(nbytes > 0, "LoFTR needs H, W >= 32 (got ", H, "x", W, ")");
    c10::DeviceGuard g(frames.device());
    auto o = frames.options().dtype(at::kFloat);
    const int64_t H8 = H / 8 * 8, W8 = W / 8 * 8;
    Tensor coarse = at::empty({B, (H8 / 8) * (W8 / 8), 256}, o), fine = at::empty({B, (H8 / 2) * (W8 / 2), 128}, o);
    Tensor ws = workspace(nbytes, frames);
    check_rc(mlg_loftr_features(&s, cp<uint8_t>(frames), (int)B, (int)H, (int)W, (int)C, (long)(H * W * C),
                                ws.data_ptr(), (size_t)ws.numel(), mp<float>(coarse), mp<float>(fine),
                                stream_of(frames)),
             "mlg_loftr_features");
    return {coarse, fine};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> loftr_match(const Tensor& coarse, const Tensor& fine, const Tensor& pa,
                                                       const Tensor& pb, const Tensor& pe, at::TensorList w, int64_t H,
                                                       int64_t W) {
    want(coarse, at::kFloat, "coarse");
    want(fine, at::kFloat, "fine");
    want(pe, at::kFloat, "pe");
    want(pa, at::kInt, "pair_a", false);
    want(pb, at::kInt, "pair_b", false);
    const int64_t P = pa.numel(), F = coarse.size(0), L = (H / 8) * (W / 8);
    TORCH_CHECK(pb.numel() == P && P > 0, "pair lists must be non-empty and of equal length");
    TORCH_CHECK(coarse.dim() == 3 && coarse.size(1) == L && coarse.size(2) == 256, "coarse must be [F, H/8*W/8, 256]");
    TORCH_CHECK(fine.dim() == 3 && fine.size(0) == F && fine.size(1) == (H / 2) * (W / 2) && fine.size(2) == 128,
                "fine must be [F, H/2*W/2, 128]");
    TORCH_CHECK(pe.numel() == L * 256, "pe must be [H/8*W/8, 256]");
    const int32_t* a = pa.data_ptr<int32_t>();
    const int32_t* b = pb.data_ptr<int32_t>();
    for (int64_t p = 0; p < P; ++p)
        TORCH_CHECK(a[p] >= 0 && a[p] < F && b[p] >= 0 && b[p] < F, "pair ", p, " indexes a missing frame");
    const mlg_loftr_weights s = loftr_weights(w, coarse.device());
    const size_t nbytes = mlg_loftr_match_ws_bytes((int)P, (int)H, (int)W);
    TORCH_CHECK(nbytes > 0, "LoFTR needs H, W >= 32 and multiples of 8");
    c10::DeviceGuard g(coarse.device());
    auto o = coarse.options();
    Tensor counts = at::empty({P}, o.dtype(at::kInt));
    Tensor k0 = at::zeros({P, L, 2}, o), k1 = at::zeros({P, L, 2}, o), cf = at::zeros({P, L}, o);
    Tensor ws = workspace(nbytes, coarse);
    check_rc(mlg_loftr_match(&s, cp<float>(coarse), cp<float>(fine), (int)H, (int)W, a, b, (int)P, cp<float>(pe),
                             ws.data_ptr(), (size_t)ws.numel(), mp<int32_t>(counts), mp<float>(k0), mp<float>(k1),
                             mp<float>(cf), stream_of(coarse)),
             "mlg_loftr_match");
    return {counts, k0, k1, cf};
}

// --------------------------------------------------------------- SuperGlue
// bin_score arrives as a double beside the list
std::tuple<Tensor, Tensor, Tensor> superglue(const Tensor& kpts, const Tensor& scores, const Tensor& desc,
                                             const Tensor& counts, const Tensor& pair_a, const Tensor& pair_b,
                                             at::TensorList w, double bin_score, int64_t W, int64_t H, int64_t iters,
                                             double thr) {
    want(kpts, at::kFloat, "kpts");
    want(scores, at::kFloat, "scores");
    want(desc, at::kFloat, "desc");
    want(counts, at::kInt, "counts", false);
    want(pair_a, at::kInt, "pair_a", false);
    want(pair_b, at::kInt, "pair_b", false);
    const int64_t F = kpts.size(0), kmax = kpts.size(1), P = pair_a.numel();
    TORCH_CHECK(kpts.dim() == 3 && kpts.size(2) == 2 && desc.dim() == 3 && desc.size(0) == F &&
                    desc.size(1) == kmax && desc.size(2) == 256 && scores.numel() == F * kmax,
                "kpts [F, kmax, 2] / scores [F, kmax] / desc [F, kmax, 256]");
    TORCH_CHECK(counts.numel() == F && pair_b.numel() == P && P > 0, "counts [F], pair_a / pair_b [P]");
    const int32_t* cn = cp<int32_t>(counts);
    for (int64_t f = 0; f < F; ++f) TORCH_CHECK(cn[f] >= 0 && cn[f] <= kmax, "counts out of range");
    mlg_sg_weights s = MLG_STRUCT_INIT(mlg_sg_weights);
    fill_weights(wt::sg_table(), "superglue", w, &s, kpts.device());
    s.bin_score = (float)bin_score;
    const size_t nbytes = mlg_superglue_workspace_bytes((int)P, (int)kmax);
    c10::DeviceGuard g(kpts.device());
    auto o = kpts.options();
    Tensor m = at::empty({P, kmax, 2}, o.dtype(at::kInt)), sc = at::empty({P, kmax}, o.dtype(at::kFloat));
    Tensor n = at::empty({P}, o.dtype(at::kInt));
    Tensor ws = workspace(nbytes, kpts);
    check_rc(mlg_superglue(&s, cp<float>(kpts), cp<float>(scores), cp<float>(desc), cn, (int)F, (int)kmax, (int)W,
                           (int)H, cp<int32_t>(pair_a), cp<int32_t>(pair_b), (int)P, (int)iters, (float)thr,
                           ws.data_ptr(), (size_t)ws.numel(), mp<int32_t>(m), mp<float>(sc), mp<int32_t>(n),
                           stream_of(kpts)),
             "mlg_superglue");
    return {m, sc, n};
}

// CricaVPR.rerank_candidates at scale: feats f32 [F, L, D], query / cand int32 [P] -> scores f32 [P]
Tensor xcorr_batch(const Tensor& feats, const Tensor& query, const Tensor& cand) {
    want(feats, at::kFloat, "feats");
    want(query, at::kInt, "query");
    want(cand, at::kInt, "cand");
    TORCH_CHECK(feats.dim() == 3 && feats.size(2) % 4 == 0, "feats [F, L, D] with D % 4 == 0");
    TORCH_CHECK(query.numel() == cand.numel(), "query / cand [P]");
    const int64_t F = feats.size(0), L = feats.size(1), D = feats.size(2), P = query.numel();
    c10::DeviceGuard g(feats.device());
    Tensor out = at::empty({P}, feats.options());
    if (P == 0) return out;
    Tensor ws = workspace(mlg_xcorr_batch_workspace_bytes((int)F, (int)L, (int)D, (int)P), feats);
    check_rc(mlg_xcorr_batch(cp<float>(feats), (int)F, (int)L, (int)D, cp<int32_t>(query), cp<int32_t>(cand), (int)P,
                             ws.data_ptr(), (size_t)ws.numel(), mp<float>(out), stream_of(feats)),
             "mlg_xcorr_batch");
    return out;
}

// CricaVPR.rerank_candidates over knn_gate's lists: feats f32 [F, L, D]; idx / sim / mask [Q, k], count [Q];
// cached uint8 [F] or none; totals int64 [1] or none -> r_idx, r_sim, r_cross, r_score [Q, top_k], r_count [Q]
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> rerank_gate(const Tensor& feats, const Tensor& idx,
                                                               const Tensor& sim, const c10::optional<Tensor>& mask,
                                                               const Tensor& count, int64_t top_k, int64_t q0,
                                                               const c10::optional<Tensor>& cached,
                                                               const c10::optional<Tensor>& totals) {
    want(feats, at::kFloat, "feats");
    want(idx, at::kInt, "idx");
    want(sim, at::kFloat, "sim");
    want(count, at::kInt, "count");
    TORCH_CHECK(feats.dim() == 3 && feats.size(2) % 4 == 0, "feats [F, L, D] with D % 4 == 0");
    TORCH_CHECK(idx.dim() == 2 && sim.sizes() == idx.sizes() && count.numel() == idx.size(0),
                "idx / sim [Q, k], count [Q]");
    const int64_t F = feats.size(0), L = feats.size(1), D = feats.size(2), Q = idx.size(0), k = idx.size(1);
    TORCH_CHECK(k >= 1 && k <= 64, "rerank_gate: k must be in [1, 64]");
    TORCH_CHECK(top_k >= 1 && top_k <= k, "rerank_gate: top_k must be in [1, k]");
    TORCH_CHECK(q0 >= 0 && q0 + Q <= F, "query rows out of range");
    const bool has_mask = mask.has_value() && mask->defined();
    const bool has_cached = cached.has_value() && cached->defined();
    const bool has_totals = totals.has_value() && totals->defined();
    if (has_mask) {
        want(*mask, at::kByte, "mask");
        TORCH_CHECK(mask->sizes() == idx.sizes(), "mask must be uint8 [Q, k]");
    }
    if (has_cached) {
        want(*cached, at::kByte, "cached");
        TORCH_CHECK(cached->numel() == F, "cached must be uint8 [F]");
    }
    if (has_totals) {
        want(*totals, at::kLong, "totals");
        TORCH_CHECK(totals->numel() == 1, "totals must be int64 [1]");
    }
    c10::DeviceGuard g(feats.device());
    auto o = feats.options();
    Tensor r_idx = at::empty({Q, top_k}, o.dtype(at::kInt)), r_sim = at::empty({Q, top_k}, o.dtype(at::kFloat));
    Tensor r_cross = at::empty({Q, top_k}, o.dtype(at::kFloat)), r_score = at::empty({Q, top_k}, o.dtype(at::kDouble));
    Tensor r_count = at::empty({Q}, o.dtype(at::kInt));
    if (Q == 0) return {r_idx, r_sim, r_cross, r_score, r_count};
    const size_t nbytes = mlg_rerank_workspace_bytes((int)F, (int)L, (int)D, (int)Q, (int)k);
    TORCH_CHECK(nbytes > 0, "rerank_gate: unsupported shape F=", F, " L=", L, " D=", D, " Q=", Q, " k=", k);
    Tensor ws = workspace(nbytes, feats);
    check_rc(mlg_rerank_gate(cp<float>(feats), (int)F, (int)L, (int)D, (int)q0, (int)Q, (int)k, cp<int32_t>(idx),
                             cp<float>(sim), has_mask ? cp<uint8_t>(*mask) : nullptr, cp<int32_t>(count),
                             has_cached ? cp<uint8_t>(*cached) : nullptr, (int)top_k, ws.data_ptr(),
                             (size_t)ws.numel(), mp<int32_t>(r_idx), mp<float>(r_sim), mp<float>(r_cross),
                             mp<double>(r_score), mp<int32_t>(r_count),
                             has_totals ? mp<unsigned long long>(*totals) : nullptr, stream_of(feats)),
             "mlg_rerank_gate");
    return {r_idx, r_sim, r_cross, r_score, r_count};
}

// The sequence-consistency check over knn_gate's lists (mlg_seq_gate states the rule): desc f32 [N, D],
// t f64 [N], floor int64 [N], has_floor uint8 [N]; idx / sim / mask [Q, k], count [Q]; totals int64 [1] or
// none -> s_score f64, s_dir int8, s_terms int32, keep uint8, all [Q, k]
std::tuple<Tensor, Tensor, Tensor, Tensor> seq_gate(const Tensor& desc, const Tensor& t, const Tensor& floor,
                                                    const Tensor& has_floor, const Tensor& idx, const Tensor& sim,
                                                    const c10::optional<Tensor>& mask, const Tensor& count,
                                                    int64_t radius, double threshold, double min_gap,
                                                    int64_t min_terms, int64_t q0,
                                                    const c10::optional<Tensor>& totals) {
    want(desc, at::kFloat, "desc");
    want(t, at::kDouble, "t");
    want(floor, at::kLong, "floor");
    want(has_floor, at::kByte, "has_floor");
    want(idx, at::kInt, "idx");
    want(sim, at::kFloat, "sim");
    want(count, at::kInt, "count");
    TORCH_CHECK(desc.dim() == 2, "desc [N, D]");
    const int64_t N = desc.size(0), D = desc.size(1);
    TORCH_CHECK(t.numel() == N && floor.numel() == N && has_floor.numel() == N, "t / floor / has_floor [N]");
    TORCH_CHECK(idx.dim() == 2 && sim.sizes() == idx.sizes() && count.numel() == idx.size(0),
                "idx / sim [Q, k], count [Q]");
    const int64_t Q = idx.size(0), k = idx.size(1);
    TORCH_CHECK(k >= 1 && k <= 64, "seq_gate: k must be in [1, 64]");
    TORCH_CHECK(radius >= 1 && radius <= 7, "seq_gate: radius must be in [1, 7]");
    TORCH_CHECK(min_terms >= 1, "seq_gate: min_terms must be >= 1");
    TORCH_CHECK(q0 >= 0 && q0 + Q <= N, "query rows out of range");
    const bool has_mask = mask.has_value() && mask->defined();
    const bool has_totals = totals.has_value() && totals->defined();
    if (has_mask) {
        want(*mask, at::kByte, "mask");
        TORCH_CHECK(mask->sizes() == idx.sizes(), "mask must be uint8 [Q, k]");
    }
    if (has_totals) {
        want(*totals, at::kLong, "totals");
        TORCH_CHECK(totals->numel() == 1, "totals must be int64 [1]");
    }
    c10::DeviceGuard g(desc.device());
    auto o = desc.options();
    Tensor s_score = at::empty({Q, k}, o.dtype(at::kDouble)), s_dir = at::empty({Q, k}, o.dtype(at::kChar));
    Tensor s_terms = at::empty({Q, k}, o.dtype(at::kInt)), keep = at::empty({Q, k}, o.dtype(at::kByte));
    if (Q == 0) return {s_score, s_dir, s_terms, keep};
    const size_t nbytes = mlg_seq_workspace_bytes((int)N, (int)D, (int)Q, (int)k);
    TORCH_CHECK(nbytes > 0, "seq_gate: unsupported shape N=", N, " D=", D, " Q=", Q, " k=", k);
    Tensor ws = workspace(nbytes, desc);
    check_rc(mlg_seq_gate(cp<float>(desc), (int)N, (int)D, cp<double>(t), cp<int64_t>(floor), cp<uint8_t>(has_floor),
                          (int)q0, (int)Q, (int)k, cp<int32_t>(idx), cp<float>(sim),
                          has_mask ? cp<uint8_t>(*mask) : nullptr, cp<int32_t>(count), (int)radius, min_gap,
                          (int)min_terms, threshold, ws.data_ptr(), (size_t)ws.numel(), mp<double>(s_score),
                          mp<int8_t>(s_dir), mp<int32_t>(s_terms), mp<uint8_t>(keep),
                          has_totals ? mp<unsigned long long>(*totals) : nullptr, stream_of(desc)),
             "mlg_seq_gate");
    return {s_score, s_dir, s_terms, keep};
}

// knn_gate as keyframes arrive (mlg_knn_append states the rule).  The state tensors are the caller's and
// are updated in place: xn f32 [cap, D] (rows [0, n_new) normalised), t f64 / floor int64 / has_floor uint8
// [cap], idx int32 / sim f32 / valid uint8 [cap, k], count int32 [cap] -> inserted int32 [n_old],
// evicted_idx int32 [n_old, k], n_evicted int32 [n_old]
std::tuple<Tensor, Tensor, Tensor> knn_append(const Tensor& xn, const Tensor& t, const Tensor& floor,
                                              const Tensor& has_floor, const Tensor& idx, const Tensor& sim,
                                              const Tensor& valid, const Tensor& count, int64_t n_old, int64_t n_new,
                                              double min_gap, double thr, int64_t k, bool gating, int64_t phases) {
    want(xn, at::kFloat, "xn");
    want(t, at::kDouble, "t");
    want(floor, at::kLong, "floor");
    want(has_floor, at::kByte, "has_floor");
    want(idx, at::kInt, "idx");
    want(sim, at::kFloat, "sim");
    want(valid, at::kByte, "valid");
    want(count, at::kInt, "count");
    TORCH_CHECK(xn.dim() == 2, "xn must be [cap, D]");
    const int64_t cap = xn.size(0), D = xn.size(1);
    TORCH_CHECK(t.numel() == cap && floor.numel() == cap && has_floor.numel() == cap,
                "t / floor / has_floor must be [cap]");
    TORCH_CHECK(idx.dim() == 2 && idx.size(0) == cap && idx.size(1) == k && sim.sizes() == idx.sizes() &&
                    valid.sizes() == idx.sizes() && count.numel() == cap,
                "idx / sim / valid must be [cap, k], count [cap]");
    TORCH_CHECK(k >= 1 && k <= 32, "knn_append: k must be in [1, 32]");
    TORCH_CHECK(D % 4 == 0, "knn_append: D must be a multiple of 4");
    TORCH_CHECK(n_old >= 0 && n_old < n_new && n_new <= cap, "knn_append: need 0 <= n_old < n_new <= cap");
    for (const Tensor* x : {&t, &floor, &has_floor, &idx, &sim, &valid, &count})
        TORCH_CHECK(x->device() == xn.device(), "knn_append: every state tensor must be on ", xn.device());
    c10::DeviceGuard g(xn.device());
    auto o = xn.options().dtype(at::kInt);
    Tensor inserted = at::empty({n_old}, o), evicted = at::empty({n_old, k}, o), n_evicted = at::empty({n_old}, o);
    const size_t nbytes = mlg_knn_append_workspace_bytes((int)n_old, (int)n_new, (int)D, (int)k);
    TORCH_CHECK(nbytes > 0, "knn_append: unsupported shape n_old=", n_old, " n_new=", n_new, " D=", D, " k=", k);
    Tensor ws = workspace(nbytes, xn);
    TORCH_CHECK(phases >= 1 && phases <= 3, "knn_append: phases must be 1 (update), 2 (fresh) or 3 (both)");
    check_rc(mlg_op_knn_append_phases(cp<float>(xn), (int)n_old, (int)n_new, (int)D, cp<double>(t), cp<int64_t>(floor),
                            cp<uint8_t>(has_floor), min_gap, (float)thr, (int)k, gating ? 1 : 0, ws.data_ptr(),
                            (size_t)ws.numel(), mp<int32_t>(idx), mp<float>(sim), mp<uint8_t>(valid),
                            mp<int32_t>(count), mp<int32_t>(inserted), mp<int32_t>(evicted), mp<int32_t>(n_evicted),
                            (int)phases, stream_of(xn)),
             "mlg_knn_append");
    return {inserted, evicted, n_evicted};
}

// --------------------------------------------------------------- LightGlue
std::tuple<Tensor, Tensor, Tensor, Tensor> lightglue(const Tensor& kpts, const Tensor& desc, const Tensor& counts,
                                                     const Tensor& pair_a, const Tensor& pair_b, at::TensorList w,
                                                     double depth_conf, double width_conf, double filter_thr,
                                                     int64_t pruning_min) {
    want(kpts, at::kFloat, "kpts");
    want(desc, at::kFloat, "desc");
    want(counts, at::kInt, "counts", false);
    want(pair_a, at::kInt, "pair_a", false);
    want(pair_b, at::kInt, "pair_b", false);
    const int64_t F = kpts.size(0), kmax = kpts.size(1), P = pair_a.numel();
    TORCH_CHECK(kpts.dim() == 3 && kpts.size(2) == 2 && desc.dim() == 3 && desc.size(0) == F &&
                    desc.size(1) == kmax && desc.size(2) == 256, "kpts [F, kmax, 2] / desc [F, kmax, 256]");
    TORCH_CHECK(counts.numel() == F && pair_b.numel() == P, "counts [F], pair_a / pair_b [P]");
    const int32_t* pa = cp<int32_t>(pair_a);
    const int32_t* pb = cp<int32_t>(pair_b);
    const int32_t* cn = cp<int32_t>(counts);
    for (int64_t p = 0; p < P; ++p)
        TORCH_CHECK(pa[p] >= 0 && pa[p] < F && pb[p] >= 0 && pb[p] < F, "pair frame index out of range");
    for (int64_t f = 0; f < F; ++f) TORCH_CHECK(cn[f] >= 0 && cn[f] <= kmax, "counts out of range");
    mlg_lg_weights s = MLG_STRUCT_INIT(mlg_lg_weights);
    fill_weights(wt::lg_table(), "lightglue", w, &s, kpts.device());
    const size_t nbytes = mlg_lightglue_workspace_bytes((int)P, (int)kmax);
    TORCH_CHECK(nbytes > 0, "LightGlue supports up to 2048 keypoints per image (got ", kmax, ")");
    c10::DeviceGuard g(kpts.device());
    auto o = kpts.options();
    Tensor m = at::empty({P, kmax, 2}, o.dtype(at::kInt)), sc = at::empty({P, kmax}, o.dtype(at::kFloat));
    Tensor n = at::empty({P}, o.dtype(at::kInt));
    Tensor stop = at::zeros({P}, counts.options());
    if (P == 0) return {m, sc, n, stop};
    Tensor ws = workspace(nbytes, kpts);
    check_rc(mlg_lightglue(&s, cp<float>(kpts), cp<float>(desc), cn, (int)F, (int)kmax, pa, pb, (int)P,
                           (float)depth_conf, (float)width_conf, (float)filter_thr, (int)pruning_min, ws.data_ptr(),
                           (size_t)ws.numel(), mp<int32_t>(m), mp<float>(sc), mp<int32_t>(n), mp<int32_t>(stop),
                           stream_of(kpts)),
             "mlg_lightglue");
    return {m, sc, n, stop};
}

std::tuple<Tensor, Tensor, Tensor> lg_orient(const Tensor& m, const Tensor& sc, const Tensor& n, const Tensor& rows,
                                             const Tensor& swap) {
    want(m, at::kInt, "matches");
    want(sc, at::kFloat, "scores");
    want(n, at::kInt, "num_matches");
    want(rows, at::kInt, "rows");
    want(swap, at::kByte, "swap");
    TORCH_CHECK(m.dim() == 3 && m.size(2) == 2 && sc.size(0) == m.size(0) && n.numel() == m.size(0),
                "matches [R, kmax, 2], scores [R, kmax], num [R]");
    TORCH_CHECK(rows.numel() == swap.numel(), "rows / swap sizes differ");
    const int64_t P = rows.numel(), kmax = m.size(1);
    c10::DeviceGuard g(m.device());
    Tensor mo = at::empty({P, kmax, 2}, m.options()), so = at::empty({P, kmax}, sc.options());
    Tensor no = at::empty({P}, n.options());
    check_rc(mlg_lg_orient_matches(cp<int32_t>(m), cp<float>(sc), cp<int32_t>(n), cp<int32_t>(rows),
                                   cp<uint8_t>(swap), (int)P, (int)kmax, mp<int32_t>(mo), mp<float>(so),
                                   mp<int32_t>(no), stream_of(m)),
             "mlg_lg_orient_matches");
    return {mo, so, no};
}

// ------------------------------------------------------------------ RANSAC
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> ransac_epipolar(const Tensor& k1, const Tensor& k2,
                                                                   const Tensor& offs, const c10::optional<Tensor>& K,
                                                                   int64_t k_stride, double thr, int64_t hypotheses,
                                                                   int64_t seed, bool with_pose) {
    want(k1, at::kFloat, "k1");
    want(k2, at::kFloat, "k2");
    want(offs, at::kInt, "offs");
    const bool has_k = K.has_value() && K->defined();
    if (has_k) want(*K, at::kDouble, "K");
    const int64_t P = offs.numel() - 1, S = k1.size(0);
    TORCH_CHECK(P >= 1 && k1.dim() == 2 && k1.size(1) == 2 && k2.sizes() == k1.sizes(), "ransac shapes");
    TORCH_CHECK(!has_k || K->numel() >= 9 + (P - 1) * k_stride, "K too small for the pairs");
    const size_t nbytes = mlg_ransac_workspace_bytes((int)P, (long)S, (int)hypotheses);
    TORCH_CHECK(nbytes > 0, "bad RANSAC shape");
    c10::DeviceGuard g(k1.device());
    auto o = k1.options();
    Tensor model = at::empty({P, 9}, o.dtype(at::kDouble)), mask = at::empty({std::max<int64_t>(S, 1)}, o.dtype(at::kByte));
    Tensor inl = at::empty({P}, o.dtype(at::kInt)), status = at::empty({P}, o.dtype(at::kInt));
    Tensor pose = (with_pose && has_k) ? at::empty({P, 16}, o.dtype(at::kDouble)) : at::empty({0}, o.dtype(at::kDouble));
    Tensor ws = workspace(nbytes, k1);
    check_rc(mlg_ransac_epipolar(cp<float>(k1), cp<float>(k2), cp<int32_t>(offs), (int)P, (long)S,
                                 has_k ? cp<double>(*K) : nullptr, (int)k_stride, thr, (int)hypotheses, (uint64_t)seed,
                                 ws.data_ptr(), (size_t)ws.numel(), mp<double>(model), mp<uint8_t>(mask),
                                 mp<int32_t>(inl), pose.numel() ? mp<double>(pose) : nullptr, mp<int32_t>(status),
                                 stream_of(k1)),
             "mlg_ransac_epipolar");
    return {model, mask.narrow(0, 0, S), inl, pose, status};
}

Tensor recover_pose(const Tensor& k1, const Tensor& k2, const Tensor& offs, const Tensor& K, int64_t k_stride,
                    const Tensor& E, const Tensor& mask) {
    want(k1, at::kFloat, "k1");
    want(k2, at::kFloat, "k2");
    want(offs, at::kInt, "offs");
    want(K, at::kDouble, "K");
    want(E, at::kDouble, "E");
    want(mask, at::kByte, "mask");
    const int64_t P = offs.numel() - 1;
    TORCH_CHECK(P >= 1 && E.numel() == 9 * P, "E must be [P, 9]");
    c10::DeviceGuard g(k1.device());
    Tensor pose = at::empty({P, 16}, k1.options().dtype(at::kDouble));
    check_rc(mlg_recover_pose(cp<float>(k1), cp<float>(k2), cp<int32_t>(offs), (int)P, cp<double>(K), (int)k_stride,
                              cp<double>(E), cp<uint8_t>(mask), mp<double>(pose), stream_of(k1)),
             "mlg_recover_pose");
    return pose;
}

// --------------------------------------------------------------- ResNet-50
Tensor resnet50(const Tensor& frames, at::TensorList w, int64_t descriptor_dim) {
    want(frames, at::kByte, "frames");
    TORCH_CHECK(frames.dim() == 4, "frames must be [B, H, W, C]");
    mlg_rn_weights s = MLG_STRUCT_INIT(mlg_rn_weights);
    fill_weights(wt::rn_table(), "resnet50", w, &s, frames.device());
    const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2), C = frames.size(3);
    c10::DeviceGuard g(frames.device());
    Tensor out = at::empty({B, descriptor_dim}, frames.options().dtype(at::kFloat));
    Tensor ws = workspace(mlg_resnet50_workspace_bytes((int)B, (int)H, (int)W), frames);
    check_rc(mlg_resnet50_forward(&s, cp<uint8_t>(frames), (int)B, (int)H, (int)W, (int)C, (long)(H * W * C),
                                  (int)descriptor_dim, ws.data_ptr(), (size_t)ws.numel(), mp<float>(out),
                                  stream_of(frames)),
             "mlg_resnet50_forward");
    return out;
}

Tensor pillow_resize_224(const Tensor& frames) {
    want(frames, at::kByte, "frames");
    const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2), C = frames.size(3);
    c10::DeviceGuard g(frames.device());
    Tensor out = at::empty({B, 224, 224, 3}, frames.options());
    Tensor ws = workspace(mlg_resnet50_workspace_bytes((int)B, (int)H, (int)W), frames);
    check_rc(mlg_op_pillow_resize_224(cp<uint8_t>(frames), (int)B, (int)H, (int)W, (int)C, (long)(H * W * C),
                                      ws.data_ptr(), (size_t)ws.numel(), mp<uint8_t>(out), stream_of(frames)),
             "mlg_op_pillow_resize_224");
    return out;
}

// ------------------------------------------------------------------ MixVPR
// frames uint8 [B, H, W, C] -> desc f32 [B, 4096]
Tensor mixvpr_forward(const Tensor& frames, at::TensorList trunk, at::TensorList head, int64_t max_batch) {
    const Frames f = frames_of(frames);
    TORCH_CHECK(max_batch > 0, "max_batch must be positive");
    mlg_mixvpr_weights s = MLG_STRUCT_INIT(mlg_mixvpr_weights);
    fill_weights(wt::mixvpr_trunk_table(), "mixvpr trunk", trunk, &s, frames.device());
    fill_weights(wt::mixvpr_head_table(), "mixvpr head", head, &s, frames.device());
    c10::DeviceGuard g(frames.device());
    Tensor desc = at::empty({f.B, MLG_MIXVPR_DIM}, frames.options().dtype(at::kFloat));
    Tensor ws = workspace(mlg_mixvpr_workspace_bytes((int)std::min(f.B, max_batch), f.H, f.W), frames);
    for_chunks(f.B, max_batch, "mlg_mixvpr_forward", [&](int64_t b0, int nb) {
        return mlg_mixvpr_forward(&s, f.p + b0 * f.stride, nb, f.H, f.W, f.C, f.stride, ws.data_ptr(),
                                  (size_t)ws.numel(), mp<float>(desc) + b0 * MLG_MIXVPR_DIM, stream_of(frames));
    });
    return desc;
}

// f32 layer3 features [B, 400, 1024] (NHWC) -> desc f32 [B, 4096]
Tensor mixvpr_head(const Tensor& feat, at::TensorList head) {
    want(feat, at::kFloat, "features");
    TORCH_CHECK(feat.dim() == 3 && feat.size(1) == 400 && feat.size(2) == 1024, "features must be [B, 400, 1024]");
    mlg_mixvpr_weights s = MLG_STRUCT_INIT(mlg_mixvpr_weights);
    fill_weights(wt::mixvpr_head_table(), "mixvpr head", head, &s, feat.device());
    c10::DeviceGuard g(feat.device());
    Tensor desc = at::empty({feat.size(0), MLG_MIXVPR_DIM}, feat.options());
    check_rc(mlg_op_mixvpr_head(&s, cp<float>(feat), (int)feat.size(0), mp<float>(desc), stream_of(feat)),
             "mlg_op_mixvpr_head");
    return desc;
}

// frames uint8 [B, H, W, C] -> f32 [B, 320, 320, 3] (RGB, normalised)
Tensor mixvpr_preprocess(const Tensor& frames) {
    want(frames, at::kByte, "frames");
    TORCH_CHECK(frames.dim() == 4, "frames must be [B, H, W, C]");
    const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2), C = frames.size(3);
    c10::DeviceGuard g(frames.device());
    Tensor out = at::empty({B, MLG_MIXVPR_SIZE, MLG_MIXVPR_SIZE, 3}, frames.options().dtype(at::kFloat));
    check_rc(mlg_op_mixvpr_preprocess(cp<uint8_t>(frames), (int)B, (int)H, (int)W, (int)C, (long)(H * W * C),
                                      mp<float>(out), stream_of(frames)),
             "mlg_op_mixvpr_preprocess");
    return out;
}

// ------------------------------------------------------------------ AnyLoc
mlg_vlad_vocab vlad_vocab(const Tensor& centers) {
    want(centers, at::kFloat, "centers");
    TORCH_CHECK(centers.dim() == 2 && centers.size(1) == MLG_VIT_EMBED, "centers must be [K, 768]");
    const int64_t K = centers.size(0);
    TORCH_CHECK(K >= 16 && K <= MLG_VLAD_MAX_CLUSTERS && K % 16 == 0, "centers: K = ", K,
                " is not a multiple of 16 in 16 .. ", MLG_VLAD_MAX_CLUSTERS);
    mlg_vlad_vocab v = MLG_STRUCT_INIT(mlg_vlad_vocab);
    v.centers = cp<float>(centers);
    v.num_clusters = (int)K;
    return v;
}

// tokens f32 [B, P, 768], centers f32 [K, 768] -> (desc f32 [B, K * 768], labels int32 [B, P])
std::tuple<Tensor, Tensor> vlad(const Tensor& tokens, const Tensor& centers) {
    want(tokens, at::kFloat, "tokens");
    TORCH_CHECK(tokens.dim() == 3 && tokens.size(0) > 0 && tokens.size(1) > 0 && tokens.size(2) == MLG_VIT_EMBED,
                "tokens must be [B, P, 768]");
    const mlg_vlad_vocab v = vlad_vocab(centers);
    TORCH_CHECK(centers.device() == tokens.device(), "centers and tokens must be on one device");
    const int64_t B = tokens.size(0), P = tokens.size(1), K = centers.size(0);
    c10::DeviceGuard g(tokens.device());
    Tensor desc = at::empty({B, K * MLG_VIT_EMBED}, tokens.options());
    Tensor labels = at::empty({B, P}, tokens.options().dtype(at::kInt));
    const size_t nbytes = mlg_vlad_workspace_bytes((int)B, (int)P, (int)K);
    TORCH_CHECK(nbytes > 0 && B * P < (1LL << 31), "vlad: unsupported shape");
    Tensor ws = workspace(nbytes, tokens);
    check_rc(mlg_op_vlad(&v, cp<float>(tokens), (int)B, (int)P, ws.data_ptr(), (size_t)ws.numel(), mp<float>(desc),
                         mp<int32_t>(labels), stream_of(tokens)),
             "mlg_op_vlad");
    return {desc, labels};
}

// frames uint8 [B, H, W, C] -> desc f32 [B, K * 768]
Tensor anyloc_forward(const Tensor& frames, at::TensorList w, const Tensor& centers, int64_t image_size,
                      int64_t flags, int64_t max_batch) {
    const Frames f = frames_of(frames);
    TORCH_CHECK(f.B > 0, "frames must be [B, H, W, C]");
    TORCH_CHECK(max_batch > 0, "max_batch must be positive");
    const mlg_vit_weights s = vit_weights(w, (flags & MLG_VIT_SPLIT) != 0, image_size, frames.device());
    const mlg_vlad_vocab v = vlad_vocab(centers);
    TORCH_CHECK(centers.device() == frames.device(), "centers and frames must be on one device");
    const int64_t D = centers.size(0) * MLG_VIT_EMBED;
    c10::DeviceGuard g(frames.device());
    Tensor desc = at::empty({f.B, D}, frames.options().dtype(at::kFloat));
    const size_t nbytes = mlg_anyloc_workspace_bytes((int)std::min(f.B, max_batch), (int)image_size, v.num_clusters);
    TORCH_CHECK(nbytes > 0, "anyloc_forward: unsupported image_size / batch");
    Tensor ws = workspace(nbytes, frames);
    for_chunks(f.B, max_batch, "mlg_anyloc_forward", [&](int64_t b0, int nb) {
        return mlg_anyloc_forward(&s, &v, f.p + b0 * f.stride, nb, f.H, f.W, f.C, f.stride, (int)image_size,
                                  (int)flags, ws.data_ptr(), (size_t)ws.numel(), mp<float>(desc) + b0 * D,
                                  stream_of(frames));
    });
    return desc;
}

// One Lloyd iteration: tokens f32 [M, 768]; centers f32 [K, 768] and labels int32 [M] are
// updated in place -> (changed int64 [1], counts int32 [K])
std::tuple<Tensor, Tensor> kmeans_step(const Tensor& tokens, const Tensor& centers, const Tensor& labels) {
    want(tokens, at::kFloat, "tokens");
    TORCH_CHECK(tokens.dim() == 2 && tokens.size(0) > 0 && tokens.size(1) == MLG_VIT_EMBED, "tokens must be [M, 768]");
    const mlg_vlad_vocab v = vlad_vocab(centers);
    want(labels, at::kInt, "labels");
    TORCH_CHECK(labels.dim() == 1 && labels.size(0) == tokens.size(0), "labels must be [M]");
    TORCH_CHECK(centers.device() == tokens.device() && labels.device() == tokens.device(),
                "tokens, centers and labels must be on one device");
    const int64_t M = tokens.size(0);
    c10::DeviceGuard g(tokens.device());
    Tensor changed = at::empty({1}, tokens.options().dtype(at::kLong));
    Tensor counts = at::empty({v.num_clusters}, tokens.options().dtype(at::kInt));
    const size_t nbytes = mlg_kmeans_workspace_bytes((long)M, v.num_clusters);
    TORCH_CHECK(nbytes > 0, "kmeans_step: unsupported shape");
    Tensor ws = workspace(nbytes, tokens);
    check_rc(mlg_kmeans_step(cp<float>(tokens), (long)M, mp<float>(centers), v.num_clusters, mp<int32_t>(labels),
                             mp<int64_t>(changed), mp<int32_t>(counts), ws.data_ptr(), (size_t)ws.numel(),
                             stream_of(tokens)),
             "mlg_kmeans_step");
    return {changed, counts};
}

// ---------------------------------------------------------------- CricaVPR
mlg_crica_weights crica_weights(at::TensorList head, double gem_p, c10::Device dev) {
    mlg_crica_weights cw = MLG_STRUCT_INIT(mlg_crica_weights);
    fill_weights(wt::crica_table(), "crica", head, &cw, dev);
    cw.gem_p = (float)gem_p;
    return cw;
}

// frames uint8 [B, H, W, C] -> (desc f32 [B, 10752], local f32 [B, (S/14)^2 - 1, 768] or
// an empty tensor).  Frames [j group, (j + 1) group) form group j; calls of at most
// max_batch frames end on group boundaries.
std::tuple<Tensor, Tensor> crica_forward(const Tensor& frames, at::TensorList w, at::TensorList head, double gem_p,
                                         int64_t image_size, int64_t flags, int64_t group, int64_t max_batch,
                                         bool with_local) {
    const Frames f = frames_of(frames);
    TORCH_CHECK(f.B > 0, "frames must be [B, H, W, C]");
    TORCH_CHECK(group >= 1 && group <= MLG_CRICA_MAX_GROUP, "group must be in 1 .. ", MLG_CRICA_MAX_GROUP);
    TORCH_CHECK(max_batch >= group, "max_batch must hold one group");
    TORCH_CHECK(flags & MLG_VIT_SPLIT, "crica_forward runs the split-bf16 trunk (MLG_VIT_SPLIT)");
    const mlg_vit_weights s = vit_weights(w, true, image_size, frames.device());
    const mlg_crica_weights cw = crica_weights(head, gem_p, frames.device());
    const int64_t grid = image_size / 14, n_local = grid * grid - 1;
    const int64_t step = std::min<int64_t>(max_batch / group * group, MLG_CRICA_MAX_BATCH / group * group);
    c10::DeviceGuard g(frames.device());
    Tensor desc = at::empty({f.B, MLG_CRICA_DIM}, frames.options().dtype(at::kFloat));
    Tensor local = at::empty({with_local ? f.B : 0, n_local, MLG_VIT_EMBED}, frames.options().dtype(at::kFloat));
    const size_t nbytes = mlg_vit_workspace_bytes((int)std::min(f.B, step), (int)image_size);
    TORCH_CHECK(nbytes > 0, "crica_forward: unsupported image_size / batch");
    Tensor ws = workspace(nbytes, frames);
    for_chunks(f.B, step, "mlg_crica_forward", [&](int64_t b0, int nb) {
        return mlg_crica_forward(&s, &cw, f.p + b0 * f.stride, nb, f.H, f.W, f.C, f.stride, (int)image_size,
                                 (int)flags, (int)group, ws.data_ptr(), (size_t)ws.numel(),
                                 mp<float>(desc) + b0 * MLG_CRICA_DIM,
                                 with_local ? mp<float>(local) + b0 * n_local * MLG_VIT_EMBED : nullptr,
                                 stream_of(frames));
    });
    return {desc, local};
}

// The trunk's residual stream before the final LayerNorm: f32 [B, 1 + (S/14)^2, 768]
Tensor vit_trunk(const Tensor& frames, at::TensorList w, int64_t image_size, int64_t flags, int64_t max_batch) {
    const Frames f = frames_of(frames);
    TORCH_CHECK(f.B > 0, "frames must be [B, H, W, C]");
    TORCH_CHECK(max_batch > 0, "max_batch must be positive");
    TORCH_CHECK(flags & MLG_VIT_SPLIT, "vit_trunk runs the split-bf16 trunk (MLG_VIT_SPLIT)");
    const mlg_vit_weights s = vit_weights(w, true, image_size, frames.device());
    const int64_t grid = image_size / 14, T = grid * grid + 1;
    c10::DeviceGuard g(frames.device());
    Tensor tokens = at::empty({f.B, T, MLG_VIT_EMBED}, frames.options().dtype(at::kFloat));
    const size_t nbytes = mlg_vit_workspace_bytes((int)std::min(f.B, max_batch), (int)image_size);
    TORCH_CHECK(nbytes > 0, "vit_trunk: unsupported image_size / batch");
    Tensor ws = workspace(nbytes, frames);
    for_chunks(f.B, max_batch, "mlg_op_vit_trunk", [&](int64_t b0, int nb) {
        return mlg_op_vit_trunk(&s, f.p + b0 * f.stride, nb, f.H, f.W, f.C, f.stride, (int)image_size, (int)flags,
                                ws.data_ptr(), (size_t)ws.numel(), mp<float>(tokens) + b0 * T * MLG_VIT_EMBED,
                                stream_of(frames));
    });
    return tokens;
}

// tokens_prenorm f32 [B, 1 + g^2, 768] -> the 14 pyramid rows f32 [B, 14, 768]
Tensor crica_pool(const Tensor& tokens, const Tensor& norm_w, const Tensor& norm_b, double gem_p) {
    want(tokens, at::kFloat, "tokens");
    want(norm_w, at::kFloat, "norm_w");
    want(norm_b, at::kFloat, "norm_b");
    TORCH_CHECK(tokens.dim() == 3 && tokens.size(0) > 0 && tokens.size(2) == MLG_VIT_EMBED,
                "tokens must be [B, 1 + g^2, 768]");
    TORCH_CHECK(norm_w.numel() == MLG_VIT_EMBED && norm_b.numel() == MLG_VIT_EMBED, "norm_w / norm_b must be [768]");
    TORCH_CHECK(norm_w.device() == tokens.device() && norm_b.device() == tokens.device(),
                "tokens, norm_w and norm_b must be on one device");
    const int64_t B = tokens.size(0), T = tokens.size(1);
    int64_t grid = 0;
    while (grid * grid + 1 < T) ++grid;
    TORCH_CHECK(grid * grid + 1 == T, "tokens: ", T, " is not 1 + a square");
    c10::DeviceGuard g(tokens.device());
    Tensor out = at::empty({B, MLG_CRICA_ROWS, MLG_VIT_EMBED}, tokens.options());
    check_rc(mlg_op_crica_pool(cp<float>(tokens), cp<float>(norm_w), cp<float>(norm_b), (int)B, (int)grid,
                               (float)gem_p, mp<float>(out), stream_of(tokens)),
             "mlg_op_crica_pool");
    return out;
}

// pooled f32 [B, 14, 768] -> desc f32 [B, 10752]
Tensor crica_encoder(const Tensor& pooled, at::TensorList head, double gem_p, int64_t group) {
    want(pooled, at::kFloat, "pooled");
    TORCH_CHECK(pooled.dim() == 3 && pooled.size(0) > 0 && pooled.size(0) <= MLG_CRICA_MAX_BATCH &&
                    pooled.size(1) == MLG_CRICA_ROWS && pooled.size(2) == MLG_VIT_EMBED,
                "pooled must be [B, 14, 768], B <= ", MLG_CRICA_MAX_BATCH);
    const mlg_crica_weights cw = crica_weights(head, gem_p, pooled.device());
    const int64_t B = pooled.size(0);
    c10::DeviceGuard g(pooled.device());
    Tensor desc = at::empty({B, MLG_CRICA_DIM}, pooled.options());
    Tensor ws = workspace(MLG_CRICA_HEAD_WS_BYTES(B), pooled);
    check_rc(mlg_op_crica_encoder(&cw, cp<float>(pooled), (int)B, (int)group, ws.data_ptr(), (size_t)ws.numel(),
                                  mp<float>(desc), stream_of(pooled)),
             "mlg_op_crica_encoder");
    return desc;
}

// ---------------------------------------------------- LiDAR plane RANSAC
std::tuple<Tensor, Tensor, Tensor> plane_ransac(const Tensor& pts, const Tensor& offsets, int64_t iterations,
                                                int64_t seed, double threshold) {
    want(pts, at::kFloat, "pts");
    want(offsets, at::kInt, "offsets");
    const int64_t S = offsets.numel() - 1;
    TORCH_CHECK(S >= 1 && iterations >= 1, "plane_ransac shapes");
    c10::DeviceGuard g(pts.device());
    auto o = pts.options();
    Tensor plane = at::empty({S, 4}, o.dtype(at::kDouble)), ratio = at::empty({S}, o.dtype(at::kDouble));
    Tensor inl = at::empty({S}, o.dtype(at::kInt));
    Tensor ws = workspace(mlg_plane_ransac_workspace_bytes((int)S, (int)iterations), pts);
    check_rc(mlg_plane_ransac(cp<float>(pts), cp<int32_t>(offsets), (int)S, (int)iterations, (uint64_t)seed, threshold,
                              ws.data_ptr(), (size_t)ws.numel(), mp<double>(plane), mp<double>(ratio),
                              mp<int32_t>(inl), stream_of(pts)),
             "mlg_plane_ransac");
    return {plane, ratio, inl};
}

// ------------------------------------------------- trajectory proximity
// count + emit in one op; reads the candidate count back (output size is data-dependent)
std::tuple<Tensor, Tensor, Tensor, Tensor> proximity(const Tensor& pos, const c10::optional<Tensor>& floor,
                                                     int64_t row0, int64_t nrows, double radius, int64_t min_gap,
                                                     bool strict) {
    want(pos, at::kDouble, "pos");
    const bool hf = floor.has_value() && floor->defined();
    if (hf) want(*floor, at::kLong, "floor");
    const int64_t N = pos.size(0);
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && row0 >= 0 && nrows >= 0 && row0 + nrows <= N,
                "proximity shapes");
    c10::DeviceGuard g(pos.device());
    auto o = pos.options();
    const size_t nbytes = mlg_proximity_workspace_bytes((int)N, (int)nrows);
    TORCH_CHECK(nbytes > 0, "proximity search supports up to 65536 poses");
    Tensor ws = workspace(nbytes, pos);
    Tensor totals = at::zeros({2}, o.dtype(at::kLong));
    const int64_t* fl = hf ? cp<int64_t>(*floor) : nullptr;
    check_rc(mlg_proximity_count(cp<double>(pos), fl, (int)N, (int)row0, (int)nrows, radius, (int)min_gap,
                                 strict ? 1 : 0, ws.data_ptr(), (size_t)ws.numel(), mp<long long>(totals),
                                 stream_of(pos)),
             "mlg_proximity_count");
    const int64_t n = totals.cpu().data_ptr<int64_t>()[0];
    Tensor pairs = at::empty({n, 2}, o.dtype(at::kInt)), dist = at::empty({n}, o.dtype(at::kDouble));
    Tensor valid = at::empty({n}, o.dtype(at::kByte));
    if (n > 0)
        check_rc(mlg_proximity_emit(cp<double>(pos), fl, (int)N, (int)row0, (int)nrows, radius, (int)min_gap,
                                    strict ? 1 : 0, ws.data_ptr(), (size_t)ws.numel(), mp<int32_t>(pairs),
                                    mp<double>(dist), mp<uint8_t>(valid), stream_of(pos)),
                 "mlg_proximity_emit");
    return {pairs, dist, valid, totals};
}

// The checks every weighted op applies to its list, on any one device (host included): lets
// a machine without a GPU compare the Python packers with the tables.  "vit" / "vit_split"
// take the token count from the list's own `pos` (the ops take it from image_size).
void weights_check(std::string model, at::TensorList w) {
    union {
        mlg_vit_weights vit;
        mlg_salad_weights salad;
        mlg_crica_weights crica;
        mlg_sp_weights sp;
        mlg_lg_weights lg;
        mlg_sg_weights sg;
        mlg_rn_weights rn;
        mlg_mixvpr_weights mix;
    } s;  // scratch: only the checks matter
    const c10::optional<c10::Device> any;
    const struct {
        const char *model, *what;
        const wt::Table& (*table)();
    } fixed[] = {{"salad", "salad", wt::salad_table},
                 {"crica", "crica", wt::crica_table},
                 {"superpoint", "superpoint", wt::sp_table},
                 {"lightglue", "lightglue", wt::lg_table},
                 {"superglue", "superglue", wt::sg_table},
                 {"resnet50", "resnet50", wt::rn_table},
                 {"mixvpr_trunk", "mixvpr trunk", wt::mixvpr_trunk_table},
                 {"mixvpr_head", "mixvpr head", wt::mixvpr_head_table}};
    for (const auto& f : fixed)
        if (model == f.model) return fill_weights(f.table(), f.what, w, &s, any);
    if (model == "vit" || model == "vit_split")
        return fill_weights(wt::vit_table(model == "vit_split", tokens_of(w, MLG_VIT_EMBED)), "vit", w, &s, any);
    TORCH_CHECK(model == "loftr", "weights_check: unknown model '", model, "'");
    loftr_weights(w, any);
}

// ------------------------------------------------------------- profiling
int64_t prof_enable(int64_t mask) { return mlg_prof_enable((int)mask); }
int64_t prof_reset() { return mlg_prof_reset(); }
std::tuple<double, int64_t, double> prof_read(int64_t slot) {
    double ms = 0.0, work = 0.0;
    long n = 0;
    check_rc(mlg_prof_read((int)slot, &ms, &n), "mlg_prof_read");
    check_rc(mlg_prof_read_work((int)slot, &work), "mlg_prof_read_work");
    return {ms, (int64_t)n, work};
}


// ------------------------------------------------------------------ ORB fallback
// iparams: int32 [57] = level_w[8], level_h[8], level_features[8], level_vec_end[8],
// umax[16], gauss[7], fast_threshold, edge_threshold; scales: float32 [8] (host tensors)
mlg_orb_params orb_params(const Tensor& ip, const Tensor& fp) {
    want(ip, at::kInt, "orb iparams", false);
    want(fp, at::kFloat, "orb fparams", false);
    TORCH_CHECK(ip.numel() == 42 && fp.numel() == MLG_ORB_LEVELS + 7,
                "orb params: expected 42 ints and 8 scales + 7 Gaussian taps");
    const int32_t* v = ip.data_ptr<int32_t>();
    const float* f = fp.data_ptr<float>();
    mlg_orb_params p = MLG_STRUCT_INIT(mlg_orb_params);
    for (int l = 0; l < MLG_ORB_LEVELS; ++l) {
        p.level_w[l] = v[l];
        p.level_h[l] = v[8 + l];
        p.level_features[l] = v[16 + l];
        p.level_scale[l] = f[l];
    }
    for (int i = 0; i < 16; ++i) p.umax[i] = v[24 + i];
    for (int i = 0; i < 7; ++i) p.gauss[i] = f[MLG_ORB_LEVELS + i];
    p.fast_threshold = v[40];
    p.edge_threshold = v[41];
    return p;
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> orb_detect(Tensor frames, Tensor pattern, Tensor iparams,
                                                                      Tensor scales, int64_t max_kp) {
    want(frames, at::kByte, "frames");
    want(pattern, at::kShort, "pattern");
    TORCH_CHECK(frames.dim() == 4, "frames: [F, H, W, C] uint8");
    TORCH_CHECK(pattern.numel() == 1024, "pattern: 256 pairs x 2 points x (x, y)");
    const c10::DeviceGuard guard(frames.device());
    const mlg_orb_params p = orb_params(iparams, scales);
    const int F = (int)frames.size(0), H = (int)frames.size(1), W = (int)frames.size(2), C = (int)frames.size(3);
    const size_t wsb = mlg_orb_workspace_bytes(&p, F, H, W, (int)max_kp);
    TORCH_CHECK(wsb > 0, "orb_detect: invalid geometry");
    Tensor ws = workspace(wsb, frames);
    auto o = frames.options();
    Tensor kp = at::empty({F, max_kp, 2}, o.dtype(at::kFloat)), resp = at::empty({F, max_kp}, o.dtype(at::kFloat));
    Tensor ang = at::empty({F, max_kp}, o.dtype(at::kFloat)), lev = at::empty({F, max_kp}, o.dtype(at::kInt));
    Tensor desc = at::zeros({F, max_kp, 32}, o), cnt = at::empty({F}, o.dtype(at::kInt));
    check_rc(mlg_orb_detect(&p, cp<int16_t>(pattern), cp<uint8_t>(frames), (long)H * W * C, F, H, W, C, (int)max_kp,
                            mp<void>(ws), wsb, mp<float>(kp), mp<float>(resp), mp<float>(ang), mp<int32_t>(lev),
                            mp<uint8_t>(desc), mp<int32_t>(cnt), stream_of(frames)),
             "mlg_orb_detect");
    return {kp, resp, ang, lev, desc, cnt};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> orb_match(Tensor desc, Tensor counts, Tensor pair_a, Tensor pair_b) {
    want(desc, at::kByte, "descriptors");
    want(counts, at::kInt, "counts");
    want(pair_a, at::kInt, "pair_a");
    want(pair_b, at::kInt, "pair_b");
    TORCH_CHECK(desc.dim() == 3 && desc.size(2) == 32, "descriptors: [F, max_kp, 32]");
    const c10::DeviceGuard guard(desc.device());
    const int P = (int)pair_a.numel(), K = (int)desc.size(1);
    TORCH_CHECK(pair_b.numel() == P, "pair_a / pair_b sizes differ");
    auto o = desc.options().dtype(at::kInt);
    Tensor q = at::empty({P, K}, o), t = at::empty({P, K}, o), d = at::empty({P, K}, o), n = at::zeros({P}, o);
    if (P == 0) return {q, t, d, n};
    const size_t wsb = mlg_orb_match_workspace_bytes(P, K);
    Tensor ws = workspace(wsb, desc);
    check_rc(mlg_orb_match(cp<uint8_t>(desc), cp<int32_t>(counts), K, cp<int32_t>(pair_a), cp<int32_t>(pair_b), P,
                           mp<void>(ws), wsb, mp<int32_t>(q), mp<int32_t>(t), mp<int32_t>(d), mp<int32_t>(n),
                           stream_of(desc)),
             "mlg_orb_match");
    return {q, t, d, n};
}

// ------------------------------------------------------------ keyframe ingestion
// Host ops (CPU key): the decoders write a caller-owned host tensor, normally a pinned
// staging buffer that mlgate.ingest uploads on a side stream.
Tensor png_load_into(std::vector<std::string> paths, Tensor out, int64_t H, int64_t W, int64_t threads) {
    want(out, at::kByte, "out", false);
    const int64_t n = (int64_t)paths.size();
    TORCH_CHECK(out.numel() >= n * H * W * 3, "out: needs ", n * H * W * 3, " bytes, has ", out.numel());
    std::vector<const char*> cps(paths.size());
    for (size_t i = 0; i < paths.size(); ++i) cps[i] = paths[i].c_str();
    Tensor status = at::zeros({n}, at::TensorOptions().dtype(at::kInt));
    check_rc(mlg_png_load_bgr(cps.data(), (int)n, mp<uint8_t>(out), (int)H, (int)W, (int)threads,
                              mp<int32_t>(status)), "mlg_png_load_bgr");
    return status;
}

std::tuple<Tensor, Tensor> png_decode(std::vector<Tensor> blobs, int64_t H, int64_t W, int64_t threads) {
    const int64_t n = (int64_t)blobs.size();
    std::vector<const uint8_t*> ptrs(n);
    std::vector<size_t> lens(n);
    for (int64_t i = 0; i < n; ++i) {
        want(blobs[i], at::kByte, "blob", false);
        ptrs[i] = cp<uint8_t>(blobs[i]);
        lens[i] = (size_t)blobs[i].numel();
    }
    Tensor out = at::zeros({n, H, W, 3}, at::TensorOptions().dtype(at::kByte));
    Tensor status = at::zeros({n}, at::TensorOptions().dtype(at::kInt));
    check_rc(mlg_png_decode_bgr(ptrs.data(), lens.data(), (int)n, mp<uint8_t>(out), (int)H, (int)W, (int)threads,
                                mp<int32_t>(status)), "mlg_png_decode_bgr");
    return {out, status};
}

// JPEG: the host half fills three caller-owned host tensors (views of one pinned staging
// buffer in mlgate.ingest); image i lies at coefs + i * mlg_jpeg_coef_bytes(H, W).
size_t jpeg_check_host(int64_t n, const Tensor& coefs, const Tensor& qtabs, const Tensor& params, int64_t H,
                       int64_t W, bool device) {
    TORCH_CHECK(H > 0 && W > 0 && H <= 65535 && W <= 65535 && n <= 65535, "jpeg: bad batch ", n, " x ", H, " x ", W);
    const size_t per = mlg_jpeg_coef_bytes((int)H, (int)W);
    want(coefs, at::kShort, "coefs", device);
    want(qtabs, at::kUInt16, "qtabs", device);
    TORCH_CHECK((size_t)coefs.numel() * 2 >= (size_t)n * per, "coefs: needs ", (size_t)n * per, " bytes, has ",
                coefs.numel() * 2);
    TORCH_CHECK(qtabs.numel() >= n * 192, "qtabs: needs ", n * 192, " elements, has ", qtabs.numel());
    TORCH_CHECK(params.scalar_type() == at::kInt && params.is_contiguous() && params.numel() >= n * MLG_JPEG_PARAMS,
                "params: expected contiguous int32 with ", n * MLG_JPEG_PARAMS, " elements");
    return per;
}

Tensor jpeg_coefs_load_into(std::vector<std::string> paths, Tensor coefs, Tensor qtabs, Tensor params, int64_t H,
                            int64_t W, int64_t threads) {
    const int64_t n = (int64_t)paths.size();
    jpeg_check_host(n, coefs, qtabs, params, H, W, false);
    TORCH_CHECK(params.device().is_cpu(), "params must be a host tensor");
    std::vector<const char*> cps(paths.size());
    for (size_t i = 0; i < paths.size(); ++i) cps[i] = paths[i].c_str();
    Tensor status = at::zeros({n}, at::TensorOptions().dtype(at::kInt));
    check_rc(mlg_jpeg_coefs_load(cps.data(), (int)n, mp<int16_t>(coefs), mp<uint16_t>(qtabs), mp<int32_t>(params),
                                 (int)H, (int)W, (int)threads, mp<int32_t>(status)), "mlg_jpeg_coefs_load");
    return status;
}

Tensor jpeg_coefs_decode(std::vector<Tensor> blobs, Tensor coefs, Tensor qtabs, Tensor params, int64_t H, int64_t W,
                         int64_t threads) {
    const int64_t n = (int64_t)blobs.size();
    jpeg_check_host(n, coefs, qtabs, params, H, W, false);
    TORCH_CHECK(params.device().is_cpu(), "params must be a host tensor");
    std::vector<const uint8_t*> ptrs(n);
    std::vector<size_t> lens(n);
    for (int64_t i = 0; i < n; ++i) {
        want(blobs[i], at::kByte, "blob", false);
        ptrs[i] = cp<uint8_t>(blobs[i]);
        lens[i] = (size_t)blobs[i].numel();
    }
    Tensor status = at::zeros({n}, at::TensorOptions().dtype(at::kInt));
    check_rc(mlg_jpeg_coefs_decode(ptrs.data(), lens.data(), (int)n, mp<int16_t>(coefs), mp<uint16_t>(qtabs),
                                   mp<int32_t>(params), (int)H, (int)W, (int)threads, mp<int32_t>(status)),
             "mlg_jpeg_coefs_decode");
    return status;
}

// [status, width, height, components, luma h, luma v, supported, 0, 0] of one blob's header
Tensor jpeg_info(const Tensor& blob) {
    want(blob, at::kByte, "blob", false);
    Tensor out = at::zeros({9}, at::TensorOptions().dtype(at::kInt));
    int32_t* o = mp<int32_t>(out);
    o[0] = blob.numel() ? mlg_jpeg_info(cp<uint8_t>(blob), (size_t)blob.numel(), o + 1) : MLG_EINVAL;
    return out;
}

int64_t jpeg_coef_bytes(int64_t H, int64_t W) {
    return H > 0 && W > 0 && H <= 65535 && W <= 65535 ? (int64_t)mlg_jpeg_coef_bytes((int)H, (int)W) : 0;
}

// Device half.  The kernel indexes the coefficient buffer through `params` alone, so every
// record is checked on the host against the tensors' sizes before the launch.  `params` is
// normally the host tensor the decoder filled (checked, then uploaded); a device tensor is
// read back first (one synchronising copy of 64 B per image).
Tensor jpeg_pixels(const Tensor& coefs, const Tensor& qtabs, const Tensor& params, int64_t H, int64_t W) {
    TORCH_CHECK(params.dim() >= 1 && params.numel() % MLG_JPEG_PARAMS == 0, "params: expected [n, ", MLG_JPEG_PARAMS,
                "] int32");
    const int64_t n = params.numel() / MLG_JPEG_PARAMS;
    const size_t per = jpeg_check_host(n, coefs, qtabs, params, H, W, true);
    const c10::DeviceGuard guard(coefs.device());
    TORCH_CHECK(qtabs.device() == coefs.device(), "qtabs and coefs must be on one device");
    const Tensor host = params.device().is_cpu() ? params : params.cpu();
    check_rc(mlg_jpeg_params_check(cp<int32_t>(host), (int)n, (int)H, (int)W, per), "jpeg_pixels: parameter records");
    const Tensor dev = params.is_cuda() ? params : params.to(coefs.device());
    TORCH_CHECK(dev.device() == coefs.device(), "params and coefs must be on one device");
    Tensor out = at::empty({n, H, W, 3}, coefs.options().dtype(at::kByte));
    check_rc(mlg_jpeg_pixels(cp<int16_t>(coefs), cp<uint16_t>(qtabs), cp<int32_t>(dev), (int)n, (int)H, (int)W,
                             mp<uint8_t>(out), stream_of(coefs)), "mlg_jpeg_pixels");
    return out;
}

}  // namespace

TORCH_LIBRARY(mlgate, m) {
    m.def("vit_forward_into(Tensor frames, Tensor[] weights, int image_size, int flags, int max_batch, "
          "Tensor(a!) desc, Tensor(b!)? local) -> ()");
    m.def("dino_forward_into(Tensor frames, Tensor[] weights, int embed, int image_size, int flags, int max_batch, "
          "Tensor(a!) desc, Tensor(b!)? local) -> ()");
    m.def("dino_weights_check(Tensor[] weights, int embed, bool split) -> ()");
    m.def("salad_forward(Tensor frames, Tensor[] weights, Tensor[] salad, float dust_bin, int image_size, "
          "int max_batch) -> Tensor");
    m.def("knn_gate(Tensor desc, Tensor t, Tensor floor, Tensor has_floor, float min_gap, float thr, int k, "
          "bool gating, int q0, int Q, Tensor(a!)? totals) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("knn_query(Tensor db, Tensor q, Tensor t_db, Tensor t_q, float min_gap, int k) -> (Tensor, Tensor, Tensor)");
    m.def("row_normalize(Tensor X) -> Tensor");
    m.def("similarity(Tensor A, Tensor B) -> Tensor");
    m.def("xcorr_score(Tensor q, Tensor m) -> Tensor");
    m.def("xcorr_batch(Tensor feats, Tensor query, Tensor cand) -> Tensor");
    m.def("rerank_gate(Tensor feats, Tensor idx, Tensor sim, Tensor? mask, Tensor count, int top_k, int q0, "
          "Tensor? cached, Tensor(a!)? totals) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("seq_gate(Tensor desc, Tensor t, Tensor floor, Tensor has_floor, Tensor idx, Tensor sim, Tensor? mask, "
          "Tensor count, int radius, float threshold, float min_gap, int min_terms, int q0, Tensor(a!)? totals) "
          "-> (Tensor, Tensor, Tensor, Tensor)");
    m.def("knn_append(Tensor xn, Tensor t, Tensor floor, Tensor has_floor, Tensor(a!) idx, Tensor(b!) sim, "
          "Tensor(c!) valid, Tensor(d!) count, int n_old, int n_new, float min_gap, float thr, int k, bool gating, "
          "int phases=3) "
          "-> (Tensor, Tensor, Tensor)");
    m.def("superpoint(Tensor frames, Tensor[] weights, float detection_threshold, int max_keypoints, "
          "int nms_radius, int remove_borders, bool with_bf16) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("lightglue(Tensor kpts, Tensor desc, Tensor counts, Tensor pair_a, Tensor pair_b, Tensor[] weights, "
          "float depth_confidence, float width_confidence, float filter_threshold, int pruning_min_kpts) "
          "-> (Tensor, Tensor, Tensor, Tensor)");
    m.def("ransac_epipolar(Tensor k1, Tensor k2, Tensor offsets, Tensor? K, int k_stride, float threshold, "
          "int hypotheses, int seed, bool with_pose) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("recover_pose(Tensor k1, Tensor k2, Tensor offsets, Tensor K, int k_stride, Tensor E, Tensor mask) -> Tensor");
    m.def("resnet50(Tensor frames, Tensor[] weights, int descriptor_dim) -> Tensor");
    m.def("mixvpr_forward(Tensor frames, Tensor[] trunk, Tensor[] head, int max_batch) -> Tensor");
    m.def("mixvpr_head(Tensor features, Tensor[] head) -> Tensor");
    m.def("mixvpr_preprocess(Tensor frames) -> Tensor");
    m.def("vlad(Tensor tokens, Tensor centers) -> (Tensor, Tensor)");
    m.def("anyloc_forward(Tensor frames, Tensor[] weights, Tensor centers, int image_size, int flags, int max_batch) -> Tensor");
    m.def("kmeans_step(Tensor tokens, Tensor(a!) centers, Tensor(b!) labels) -> (Tensor, Tensor)");
    m.def("crica_forward(Tensor frames, Tensor[] weights, Tensor[] head, float gem_p, int image_size, int flags, int group, int max_batch, bool with_local) -> (Tensor, Tensor)");
    m.def("vit_trunk(Tensor frames, Tensor[] weights, int image_size, int flags, int max_batch) -> Tensor");
    m.def("crica_pool(Tensor tokens_prenorm, Tensor norm_w, Tensor norm_b, float gem_p) -> Tensor");
    m.def("crica_encoder(Tensor pooled, Tensor[] head, float gem_p, int group) -> Tensor");
    m.def("loftr_features(Tensor frames, Tensor[] weights) -> (Tensor, Tensor)");
    m.def("loftr_pack_tails(Tensor[] weights) -> Tensor");
    m.def("loftr_coarse_layer(Tensor(a!) x, Tensor(b!) cat, Tensor[] weights, int layer, int fused, int nseg, int L) -> ()");
    m.def("superglue(Tensor kpts, Tensor scores, Tensor desc, Tensor counts, Tensor pair_a, Tensor pair_b, "
          "Tensor[] weights, float bin_score, int W, int H, int iters, float threshold) -> (Tensor, Tensor, Tensor)");
    m.def("loftr_match(Tensor coarse, Tensor fine, Tensor pair_a, Tensor pair_b, Tensor pe, Tensor[] weights, int H, "
          "int W) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("pillow_resize_224(Tensor frames) -> Tensor");
    m.def("plane_ransac(Tensor pts, Tensor offsets, int iterations, int seed, float threshold) "
          "-> (Tensor, Tensor, Tensor)");
    m.def("proximity(Tensor pos, Tensor? floor, int row0, int nrows, float radius, int min_gap, bool strict) "
          "-> (Tensor, Tensor, Tensor, Tensor)");
    m.def("lg_orient(Tensor m, Tensor sc, Tensor n, Tensor rows, Tensor swap) -> (Tensor, Tensor, Tensor)");
    m.def("orb_detect(Tensor frames, Tensor pattern, Tensor iparams, Tensor scales, int max_kp) "
          "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("orb_match(Tensor desc, Tensor counts, Tensor pair_a, Tensor pair_b) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("png_load_into(str[] paths, Tensor(a!) out, int H, int W, int threads) -> Tensor");
    m.def("png_decode(Tensor[] blobs, int H, int W, int threads) -> (Tensor, Tensor)");
    m.def("jpeg_coefs_load_into(str[] paths, Tensor(a!) coefs, Tensor(b!) qtabs, Tensor(c!) params, int H, int W, "
          "int threads) -> Tensor");
    m.def("jpeg_coefs_decode(Tensor[] blobs, Tensor(a!) coefs, Tensor(b!) qtabs, Tensor(c!) params, int H, int W, "
          "int threads) -> Tensor");
    m.def("jpeg_info(Tensor blob) -> Tensor");
    m.def("jpeg_coef_bytes(int H, int W) -> int");
    m.def("jpeg_pixels(Tensor coefs, Tensor qtabs, Tensor params, int H, int W) -> Tensor");
    m.def("weights_check(str model, Tensor[] weights) -> ()");
    m.def("prof_enable(int mask) -> int");
    m.def("prof_reset() -> int");
    m.def("prof_read(int slot) -> (float, int, float)");
}

TORCH_LIBRARY_IMPL(mlgate, CUDA, m) {
    m.impl("vit_forward_into", &vit_forward_into);
    m.impl("dino_forward_into", &dino_forward_into);
    m.impl("dino_weights_check", &dino_weights_check);  // device lists; host lists: the composite kernel below
    m.impl("salad_forward", &salad_forward);
    m.impl("knn_gate", &knn_gate);
    m.impl("knn_query", &knn_query);
    m.impl("row_normalize", &row_normalize);
    m.impl("similarity", &similarity);
    m.impl("xcorr_score", &xcorr_score);
    m.impl("xcorr_batch", &xcorr_batch);
    m.impl("rerank_gate", &rerank_gate);
    m.impl("seq_gate", &seq_gate);
    m.impl("knn_append", &knn_append);
    m.impl("superpoint", &superpoint);
    m.impl("lightglue", &lightglue);
    m.impl("ransac_epipolar", &ransac_epipolar);
    m.impl("recover_pose", &recover_pose);
    m.impl("resnet50", &resnet50);
    m.impl("mixvpr_forward", &mixvpr_forward);
    m.impl("mixvpr_head", &mixvpr_head);
    m.impl("mixvpr_preprocess", &mixvpr_preprocess);
    m.impl("vlad", &vlad);
    m.impl("anyloc_forward", &anyloc_forward);
    m.impl("kmeans_step", &kmeans_step);
    m.impl("crica_forward", &crica_forward);
    m.impl("vit_trunk", &vit_trunk);
    m.impl("crica_pool", &crica_pool);
    m.impl("crica_encoder", &crica_encoder);
    m.impl("loftr_features", &loftr_features);
    m.impl("loftr_pack_tails", &loftr_pack_tails);
    m.impl("loftr_coarse_layer", &loftr_coarse_layer);
    m.impl("superglue", &superglue);
    m.impl("loftr_match", &loftr_match);
    m.impl("pillow_resize_224", &pillow_resize_224);
    m.impl("jpeg_pixels", &jpeg_pixels);
    m.impl("plane_ransac", &plane_ransac);
    m.impl("proximity", &proximity);
    m.impl("lg_orient", &lg_orient);
    m.impl("orb_detect", &orb_detect);
    m.impl("orb_match", &orb_match);
    m.impl("weights_check", &weights_check);  // device lists; host lists take the composite kernel below
}

TORCH_LIBRARY_IMPL(mlgate, CPU, m) {
    m.impl("png_load_into", &png_load_into);
    m.impl("png_decode", &png_decode);
    m.impl("jpeg_coefs_load_into", &jpeg_coefs_load_into);
    m.impl("jpeg_coefs_decode", &jpeg_coefs_decode);
    m.impl("jpeg_info", &jpeg_info);
}

TORCH_LIBRARY_IMPL(mlgate, CompositeExplicitAutograd, m) {
    m.impl("weights_check", &weights_check);
    m.impl("dino_weights_check", &dino_weights_check);
    m.impl("prof_enable", &prof_enable);
    m.impl("jpeg_coef_bytes", &jpeg_coef_bytes);
    m.impl("prof_reset", &prof_reset);
    m.impl("prof_read", &prof_read);
}
