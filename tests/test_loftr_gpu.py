"""LoFTR on the GPU (csrc/loftr.hip via torch.ops.mlgate.loftr_*) against the fp32 torch
restatement of kornia's LoFTR (oracle/loftr.py; kornia and its 'indoor' weights are
absent: seeded synthetic weights, parity unpinned against kornia itself).

Bars (bf16 MFMA convs / GEMMs against an fp32 oracle):
  * backbone (14 bf16 conv layers deep): per-cell cosine to the fp32 maps, mean >= 0.998
    and min >= 0.97 (coarse 1/8 map), mean >= 0.995 and min >= 0.95 (fine 1/2 map);
  * matching stage on the GPU's own features (stage-anchored, the oracle's f32 matching
    on the same inputs): >= 95 % of the coarse matches (i, j) shared, confidences within
    2e-2 relative, fine keypoints within 0.25 px on the shared matches;
  * end to end: >= 90 % of the oracle's coarse matches found, keypoints within 0.5 px;
  * the drop-in LoFTR.detect_and_match equals the batched path bit for bit.
"""
import numpy as np
import pytest
import torch

from mlgate import synthetic
from mlgate.loftr import LoFTRGPU
from mlgate.weights import loftr_state_dict
from oracle import loftr as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(dev):
    sd = loftr_state_dict(0)
    seq = synthetic.make_sequence(40, 8, 1)
    po = seq.place_of
    pairs = [(a, b) for a in range(40) for b in range(a + 1, 40) if po[a] == po[b]][:2]
    pairs += [(a, b) for a in range(40) for b in range(a + 1, 40) if po[a] != po[b]][:1]
    idx = sorted({i for p in pairs for i in p})
    frames = synthetic.frames_host(seq, np.arange(40))
    return sd, LoFTRGPU(device=str(dev), state_dict=sd), ol.Oracle(sd), frames, pairs, idx


def _cos(a, b):
    a, b = a.reshape(-1, a.shape[-1]).double(), b.reshape(-1, b.shape[-1]).double()
    return torch.nn.functional.cosine_similarity(a, b, dim=1)


@pytest.mark.parametrize("hw", [(480, 640), (136, 208)])
def test_backbone_matches_oracle(dev, setup, hw):
    sd, lf, orc, frames, _, _ = setup
    H, W = hw
    imgs = np.ascontiguousarray(frames[:2, :H, :W])
    c, f = lf.features(torch.from_numpy(imgs).to(dev))
    c, f = c.cpu(), f.cpu()
    for b in range(2):
        oc, of = orc.features(ol.to_gray(imgs[b]))
        cc = _cos(c[b], oc[0].permute(1, 2, 0).reshape(-1, 256))
        cf = _cos(f[b], of[0].permute(1, 2, 0).reshape(-1, 128))
        stats = (float(cc.mean()), float(cc.min()), float(cf.mean()), float(cf.min()))
        assert stats[0] >= 0.998 and stats[1] >= 0.97 and stats[2] >= 0.995 and stats[3] >= 0.95, stats


def test_matching_stage_on_gpu_features(dev, setup):
    sd, lf, orc, frames, pairs, idx = setup
    H, W = 480, 640
    fr = torch.from_numpy(frames[idx]).to(dev)
    coarse, fine = lf.features(fr)
    pos = {f: k for k, f in enumerate(idx)}
    n, k0, k1, cf = lf.match_device(coarse, fine, H, W, [pos[a] for a, _ in pairs], [pos[b] for _, b in pairs])
    n, k0, k1, cf = n.cpu().numpy(), k0.cpu().numpy(), k1.cpu().numpy(), cf.cpu().numpy()
    wc = W // 8
    for p, (a, b) in enumerate(pairs):
        c0 = coarse[pos[a]].cpu().T.reshape(1, 256, H // 8, wc)
        c1 = coarse[pos[b]].cpu().T.reshape(1, 256, H // 8, wc)
        f0 = fine[pos[a]].cpu().T.reshape(1, 128, H // 2, W // 2)
        f1 = fine[pos[b]].cpu().T.reshape(1, 128, H // 2, W // 2)
        r = orc.match_features(c0, f0, c1, f1, H)
        gi = (k0[p, :n[p], 1] / 8).astype(int) * wc + (k0[p, :n[p], 0] / 8).astype(int)  # coarse cell i
        ref = {int(i): k for k, i in enumerate(r["i_ids"].numpy())}
        shared = [k for k, i in enumerate(gi) if int(i) in ref]
        if len(ref) == 0:
            assert n[p] <= 2
            continue
        assert len(shared) >= 0.95 * len(ref), (p, len(shared), len(ref), n[p])
        ok = 0
        for k in shared:
            rk = ref[int(gi[k])]
            if np.allclose(k0[p, k], r["kpts0"][rk].numpy()) and np.abs(k1[p, k] - r["kpts1"][rk].numpy()).max() < 0.25:
                ok += 1
                assert abs(cf[p, k] - float(r["conf"][rk])) <= 2e-2 * float(r["conf"][rk])
        assert ok >= 0.95 * len(shared), (p, ok, len(shared))


def test_end_to_end_and_dropin(dev, setup):
    from mlgate.verify import LoFTR
    sd, lf, orc, frames, pairs, _ = setup
    a, b = pairs[0]
    got = lf.match_frames(torch.from_numpy(frames).to(dev), [(a, b)])[0]
    ref = orc.detect_and_match(frames[a], frames[b])
    assert len(ref[0]) > 100
    rk = {tuple(np.rint(k).astype(int)): i for i, k in enumerate(ref[0])}
    hit = [(i, rk[tuple(np.rint(k).astype(int))]) for i, k in enumerate(got[0]) if tuple(np.rint(k).astype(int)) in rk]
    assert len(hit) >= 0.9 * len(ref[0]), (len(hit), len(ref[0]), len(got[0]))
    close = sum(np.abs(got[1][i] - ref[1][j]).max() < 0.5 for i, j in hit)
    assert close >= 0.9 * len(hit)
    m = LoFTR(device=str(dev))
    m.native = True
    m._load_model()
    m._matcher = lf
    k0, k1, c = m.detect_and_match(frames[a], frames[b])
    assert np.array_equal(k0, got[0]) and np.array_equal(k1, got[1]) and np.array_equal(c, got[2])


def test_isec_frame_size_resize_path(dev, setup):
    """720 x 540 (ISEC cam, not a multiple of 8 in height): the device gray + cv2
    INTER_LINEAR resize to 720 x 536 (oracle: the C restatement of cv2.resize), matches
    and keypoints scaled back as the reference does (float64)."""
    from mlgate.verify import LoFTR
    sd, lf, orc, _, pairs, _ = setup
    seq = synthetic.make_sequence(40, 8, 1)
    a, b = pairs[0]
    fr = synthetic.frames_host(seq, np.array([a, b]), 540, 720)
    m = LoFTR(device=str(dev))
    m.native = True
    m._load_model()
    k0, k1, c = m.detect_and_match(fr[0], fr[1])
    r0, r1, rc = orc.detect_and_match(fr[0], fr[1])
    assert k0.dtype == np.float64 and len(r0) > 50
    rk = {tuple(np.rint(k * 8).astype(int)): i for i, k in enumerate(r0)}
    hit = [(i, rk[tuple(np.rint(k * 8).astype(int))]) for i, k in enumerate(k0) if tuple(np.rint(k * 8).astype(int)) in rk]
    assert len(hit) >= 0.9 * len(r0), (len(hit), len(r0), len(k0))
    assert sum(np.abs(k1[i] - r1[j]).max() < 0.5 for i, j in hit) >= 0.9 * len(hit)


def test_default_is_the_reference_lightglue_fallback(dev, monkeypatch):
    """Without kornia the reference's LoFTR warns and matches with LightGlue
    (geometric_verification.py:458-467); the drop-in does the same unless the native
    matcher is opted in (MLGATE_LOFTR_NATIVE / MLGATE_LOFTR_WEIGHTS / .native)."""
    from mlgate.verify import LightGlue, LoFTR
    monkeypatch.delenv("MLGATE_LOFTR_NATIVE", raising=False)
    monkeypatch.delenv("MLGATE_LOFTR_WEIGHTS", raising=False)
    seq = synthetic.make_sequence(40, 4, 2)
    same = [i for i in range(1, 40) if seq.place_of[i] == seq.place_of[0]]
    fr = synthetic.frames_host(seq, [0, same[0]])
    m = LoFTR(device=str(dev))
    with pytest.warns(UserWarning, match="kornia"):
        got = m.detect_and_match(fr[0], fr[1])
    ref = LightGlue(device=str(dev)).detect_and_match(fr[0], fr[1])
    assert not m._is_native
    assert all(np.array_equal(x, y) for x, y in zip(got, ref)) and len(got[0]) > 0
    # 'outdoor' without a checkpoint: the fallback too, even when native is requested
    o = LoFTR(device=str(dev), weights='outdoor')
    o.native = True
    with pytest.warns(UserWarning, match="outdoor"):
        o._load_model()
    assert not o._is_native


@pytest.mark.parametrize("B,H,W,C,k,s,N", [(2, 60, 80, 128, 3, 1, 128), (2, 61, 79, 128, 3, 2, 256),
                                           (1, 37, 53, 256, 1, 2, 256), (3, 30, 40, 256, 3, 1, 256),
                                           (1, 9, 7, 256, 3, 1, 128)])
def test_implicit_conv_matches_float64_conv(dev, B, H, W, C, k, s, N):
    """mlg_op_conv2d_nhwc (the backbone's implicit-GEMM conv, gemm_bf16.hip k_conv256) on
    bf16 inputs / weights against torch's float64 conv2d of the same bf16 values: ragged
    M (tiles of 256 output pixels), stride 2 (1x1 and 3x3), 256- and 128-wide N tiles,
    zero-padding taps on every border.  Bar: f32 accumulation, |err| <= 1e-5 of the
    output scale."""
    from mlgate import _native
    g = torch.Generator().manual_seed(B * 1000 + H + k + s)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, k, k, C, generator=g) / (k * (C ** 0.5))).to(torch.bfloat16)
    bias = torch.randn(N, generator=g) * 0.1
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    xd, wd, bd = x.to(dev), w.reshape(N, -1).contiguous().to(dev), bias.to(dev)
    zero = torch.zeros(8, dtype=torch.bfloat16, device=dev)
    out = torch.full((B, Ho, Wo, N), float("nan"), device=dev)
    P = _native.ptr
    rc = _native.lib().mlg_op_conv2d_nhwc(P(xd), P(zero), B, H, W, C, k, s, P(wd), P(bd), P(out), N,
                                          torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2),
                                     bias.double(), stride=s, padding=k // 2).permute(0, 2, 3, 1)
    got = out.cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), err


@pytest.mark.parametrize("B,H,W,C,k,s,N", [(1, 258, 258, 128, 1, 1, 512), (1, 258, 258, 128, 1, 1, 128),
                                           (2, 131, 127, 128, 3, 1, 512)])
def test_implicit_conv_walking_tiles_matches_float64_conv(dev, B, H, W, C, k, s, N):
    """test_implicit_conv_matches_float64_conv with more output tiles than CUs, so that a
    k_conv256 workgroup walks: it takes a second tile, recomputes its rows' pixel origins
    and prefetches that tile's first K-tile in the last K-step of the one before.  522
    tiles of 256 x 256 (the last M-tile of 4 rows), 261 of 256 x 128, and 260 with 3 x 3
    taps and zero padding (the last M-tile of 250 rows).  The float64 reference is the
    im2col product on the device (unfold of the same bf16 values, float64 matmul).  Same
    bar: |err| <= 1e-5 of the output scale."""
    from mlgate import _native
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    ntiles = ((B * Ho * Wo + 255) // 256) * (N // (256 if N % 256 == 0 else 128))
    assert ntiles > torch.cuda.get_device_properties(dev).multi_processor_count
    g = torch.Generator().manual_seed(B * 1000 + H + k + s)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, k, k, C, generator=g) / (k * (C ** 0.5))).to(torch.bfloat16)
    bias = torch.randn(N, generator=g) * 0.1
    xd, wd, bd = x.to(dev), w.reshape(N, -1).contiguous().to(dev), bias.to(dev)
    zero = torch.zeros(8, dtype=torch.bfloat16, device=dev)
    out = torch.full((B, Ho, Wo, N), float("nan"), device=dev)
    P = _native.ptr
    rc = _native.lib().mlg_op_conv2d_nhwc(P(xd), P(zero), B, H, W, C, k, s, P(wd), P(bd), P(out), N,
                                          torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    # unfold orders a patch (c, ty, tx): the weights go the same way
    cols = torch.nn.functional.unfold(xd.double().permute(0, 3, 1, 2), k, padding=k // 2, stride=s)
    wm = w.to(dev).double().permute(0, 3, 1, 2).reshape(N, -1)
    ref = (cols.transpose(1, 2) @ wm.T + bd.double()).reshape(B, Ho, Wo, N)
    got = out.double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), err


@pytest.mark.parametrize("layer", [0, 1])
def test_fused_coarse_tail_equals_unfused_layer(dev, setup, layer):
    """the fused coarse block tail (merge, norm1, ReLU MLP, norm2, residual in
    one lg_ffn kernel per 64-token tile) against the unfused GEMM + LayerNorm sequence on
    the same input, one self layer (0) and one cross layer (1), through
    mlg_op_loftr_coarse_layer.  Both arms round the same operands to bf16 (norm1 output,
    MLP hidden) and differ only in the GEMMs' summation order, so the residual stream x
    agrees to f32 rounding except where an intermediate lands on the other side of a bf16
    rounding boundary; the bars are the measured ones with margin."""
    sd, lf, *_ = setup
    nseg, L = 2, 600  # L > 256: the chunked K^T V partial sums as well
    g = torch.Generator(device=dev).manual_seed(5 + layer)
    x0 = torch.randn(2 * nseg * L, 256, generator=g, device=dev)
    cat0 = torch.zeros(2 * nseg * L, 512, dtype=torch.bfloat16, device=dev)
    cat0[:, :256] = x0.to(torch.bfloat16)
    out = {}
    for fused in (0, 1):
        x, cat = x0.clone(), cat0.clone()
        lf.ops.loftr_coarse_layer(x, cat, lf.weights, layer, fused, nseg, L)
        torch.cuda.synchronize()
        out[fused] = (x.double().cpu(), cat.float().double().cpu())
    xu, cu = out[0]
    xf, cf = out[1]
    scale = xu.abs().max().item()
    dx = (xf - xu).abs()
    rel = dx / xu.abs().clamp(min=1e-3 * scale)
    cell = ((xf - xu).norm(dim=1) / xu.norm(dim=1)).max().item()
    # the bf16 copy of the new x (cat[:, :256]) follows x: equal unless x moved across a rounding boundary
    same_cat = (cf[:, :256] == cu[:, :256]).double().mean().item()
    stats = {"dx_max_rel_scale": dx.max().item() / scale, "dx_median": dx.median().item(),
             "rel_p999": torch.quantile(rel.flatten()[::7].float(), 0.999).item(), "cell_rel_max": cell,
             "cat_equal": same_cat}
    print(stats)
    assert not torch.equal(xu, x0.double().cpu())
    assert cell <= 2e-3 and stats["dx_median"] <= 1e-5 * scale and same_cat >= 0.99, stats


@pytest.mark.parametrize("hw", [(480, 640), (540, 720)])
def test_split_similarity_against_exact_arm(dev, setup, hw):
    """ADVICE r05 / VERDICT r05 next 8: the coarse similarity from split-bf16 operands (the
    product default) against the exact-f32 arm (mlg_set_loftr_similarity(1)) on the SAME
    coarse features, 18 revisit pairs (three dual-softmax groups of 8), at the bench frame
    size (L = 4800) and at the ISEC frame size (720 x 540 -> 536: L = 6030, L % 4 != 0,
    which took the exact path before round 6; its S rows are now padded to 6032).  The
    mutual-nearest coarse match sets agree up to near ties, and the shared matches'
    confidences and fine keypoints agree."""
    from mlgate import _native
    sd, lf, orc, _, _, _ = setup
    H, W = hw
    seq = synthetic.make_sequence(40, 8, 1)
    po = seq.place_of
    pairs = [(a, b) for a in range(40) for b in range(a + 1, 40) if po[a] == po[b]][:18]
    idx = sorted({i for p in pairs for i in p})
    fr = torch.from_numpy(synthetic.frames_host(seq, np.array(idx), H, W)).to(dev)
    coarse, fine = lf.features(fr)
    H8, W8 = H // 8 * 8, W // 8 * 8
    pos = {f: k for k, f in enumerate(idx)}
    pa, pb = [pos[a] for a, _ in pairs], [pos[b] for _, b in pairs]
    L = _native.lib()
    out = {}
    try:
        for exact in (0, 1):
            assert L.mlg_set_loftr_similarity(exact) == 0
            out[exact] = [x.cpu().numpy() for x in lf.match_device(coarse, fine, H8, W8, pa, pb)]
    finally:
        L.mlg_set_loftr_similarity(0)
    (n0, a0, b0, c0), (n1, a1, b1, c1) = out[0], out[1]
    tot = shared = close = 0
    for p in range(len(pairs)):
        m0 = {tuple(np.rint(a0[p, k]).astype(int)): k for k in range(n0[p])}
        m1 = {tuple(np.rint(a1[p, k]).astype(int)): k for k in range(n1[p])}
        common = set(m0) & set(m1)
        tot += max(len(m0), len(m1))
        shared += len(common)
        for key in common:
            i, j = m0[key], m1[key]
            close += abs(c0[p, i] - c1[p, j]) <= 1e-3 * c1[p, j] and np.abs(b0[p, i] - b1[p, j]).max() < 0.05
        assert abs(int(n0[p]) - int(n1[p])) <= max(2, 0.01 * n1[p]), (p, n0[p], n1[p])
    print(f"{hw}: {shared} of {tot} coarse matches shared, {close} within conf 1e-3 / 0.05 px")
    assert tot > 18 * 50 and shared >= 0.99 * tot and close >= 0.99 * shared, (tot, shared, close)


def test_layer0_dedup_equals_plain_path(dev, setup):
    """coarse layer 0 (self) runs once per distinct frame of a call and its rows
    are gathered per pair side whenever a frame repeats; with all-distinct frames every pair
    side runs it itself.  Both must give the same bits.  Three frames of one place plus a
    copy of frame 0 as index 3: pairs (0, 1), (0, 2) repeat frame 0 and take the dedup path,
    pairs (0, 1), (3, 2) name four distinct rows and take the plain one.  At 480 x 640
    (L = 4800, the fixture's same-place pair and one more revisit, 283 and 279 matches): cropped to 136 x 208
    (L = 442) the seeded synthetic weights give no coarse match at all (measured: 0 and 0),
    and an all-empty comparison would show nothing."""
    sd, lf, orc, frames, pairs, _ = setup
    po = synthetic.make_sequence(40, 8, 1).place_of
    trio = [i for i in range(40) if po[i] == po[pairs[0][0]]][:3]
    assert len(trio) == 3
    assert tuple(trio[:2]) == tuple(pairs[0])
    H, W = 480, 640
    coarse, fine = lf.features(torch.from_numpy(frames[trio]).to(dev))
    coarse = torch.cat([coarse, coarse[:1]]).contiguous()
    fine = torch.cat([fine, fine[:1]]).contiguous()
    dedup = [x.cpu() for x in lf.match_device(coarse, fine, H, W, [0, 0], [1, 2])]
    plain = [x.cpu() for x in lf.match_device(coarse, fine, H, W, [0, 3], [1, 2])]
    print("matches per pair:", dedup[0].tolist(), plain[0].tolist())
    assert int(dedup[0].sum()) > 0, "no coarse match: the comparison would be vacuous"
    for name, a, b in zip(("n", "k0", "k1", "conf"), dedup, plain):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("op", ["loftr_features", "loftr_match", "loftr_coarse_layer", "loftr_pack_tails"])
def test_malformed_weight_list_is_refused(dev, setup, op):
    """Every loftr_* op checks each tensor of its list before launching (weight_tables.h)."""
    from weight_corruptions import assert_refused
    lf = setup[1]
    ops, w = lf.ops, lf.weights
    H, W = 32, 32
    L = (H // 8) * (W // 8)
    call = {
        "loftr_features": lambda b: ops.loftr_features(torch.zeros(1, H, W, 1, dtype=torch.uint8, device=dev), b),
        "loftr_match": lambda b: ops.loftr_match(torch.zeros(2, L, 256, device=dev),
                                                 torch.zeros(2, (H // 2) * (W // 2), 128, device=dev),
                                                 torch.tensor([0], dtype=torch.int32), torch.tensor([1], dtype=torch.int32),
                                                 torch.zeros(L, 256, device=dev), b, H, W),
        "loftr_coarse_layer": lambda b: ops.loftr_coarse_layer(torch.zeros(2 * L, 256, device=dev),
                                                               torch.zeros(2 * L, 512, device=dev, dtype=torch.bfloat16),
                                                               b, 0, 1, 1, L),
        "loftr_pack_tails": lambda b: ops.loftr_pack_tails(b[:129]),
    }[op]
    assert len(w) == 130
    assert_refused(call, w, 46, "coarse[0].w1")
