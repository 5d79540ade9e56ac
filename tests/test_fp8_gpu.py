"""fp8 expert weights (W8A16; BASELINE.json configs[4] dtype, the reference's unfinished --int8 slot builder.py:39-49).

Expert weights are OCP e4m3 with one scale per output row and are dequantised to bf16 at the MFMA input, so the arithmetic is
that of the bf16 kernels on the dequantised weights.  Levels:
  * the device conversion is the OCP e4m3 of torch.float8_e4m3fn (all 256 byte codes, through the kernel itself);
  * expert FFN kernels (slab form and the two grouped tiled GEMMs) against an fp64 evaluation on the dequantised weights;
  * whole encoder against the fp32 oracle with teacher-forced routing: weight quantisation error (3 mantissa bits,
    ~2.5 % rms per weight) bounded at 1e-1 of the largest logit (measured below that), routing agreement >= 85 %.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from m3asr import ops
from m3asr.config import EncoderConfig
from m3asr.engine import Engine
from m3asr.plan import pack_weights, quantize_fp8_rows, save_plan, load_plan
from m3asr.weights import make_weights
from oracle.encoder_ref import encoder_forward, sub_len


def dev(t):
    return t.cuda().contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r16(t):
    return t.float().to(torch.bfloat16).double()


def _expert_case(S, E, D, Fh, mode, seed=0):
    rng = np.random.default_rng(S + E + seed)
    g = {"uniform": rng.integers(0, E, S), "all_one": np.full(S, 3 % E), "with_dropped": rng.integers(-1, E, S)}[mode]
    g = torch.from_numpy(g.astype(np.int32))
    x = rnd(S, D, seed=1)
    w1, b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
    w2, b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
    q1, s1 = quantize_fp8_rows(w1, dims=(2,))
    q2, s2 = quantize_fp8_rows(w2, dims=(2,))
    return g, x, (w1, b1, w2, b2), (q1, s1, q2, s2)


def test_device_e4m3_decoding_matches_torch():
    """Every e4m3 byte code through the kernel: a one-row expert whose W1 row holds the 256 codes (NaN codes excluded),
    multiplied by one-hot rows, returns the decoded values exactly."""
    E, D, Fh = 1, 256, 64
    codes = torch.arange(256, dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    ok = torch.isfinite(vals)
    q1 = torch.zeros(E, Fh, D, dtype=torch.uint8)
    q1[0, 0, :] = torch.where(ok, codes, torch.zeros_like(codes))
    q1 = q1.view(torch.float8_e4m3fn)
    s1 = torch.ones(E, Fh)
    # second layer = identity on hidden unit 0 -> output column 0 (1.0 is exactly representable)
    w2 = torch.zeros(E, D, Fh)
    w2[0, 0, 0] = 1.0
    q2, s2 = w2.to(torch.float8_e4m3fn), torch.ones(E, D)
    x = torch.eye(D) * 1.0                                   # row i selects weight i
    g = torch.zeros(D, dtype=torch.int32)
    y = ops.moe_expert_ffn(dev(x), dev(g), dev(q1), torch.zeros(E, Fh).cuda(), dev(q2), torch.zeros(E, D).cuda(),
                           w1_scale=dev(s1), w2_scale=dev(s2)).cpu()
    want = F.silu(torch.where(ok, vals, torch.zeros_like(vals)).double()).float()
    # H passes through bf16 and a fast-math SiLU: 1 bf16 ulp; neighbouring e4m3 codes are >= 6 % apart (and the FNUZ
    # variant of the format would be off by a factor 2), so this pins the decoding of every code
    assert torch.allclose(y[:, 0], want, rtol=2 ** -7, atol=1e-6), float((y[:, 0] - want).abs().max())


@pytest.mark.parametrize("S,E,D,Fh,mode", [(50, 32, 512, 1024, "uniform"), (50, 32, 512, 1024, "all_one"),
                                           (200, 32, 512, 1024, "uniform"), (700, 8, 128, 256, "with_dropped"),
                                           (1090, 32, 512, 1024, "with_dropped"), (2048, 32, 512, 1024, "all_one"),
                                           (8192, 32, 512, 1024, "uniform")])
def test_fmoe_expert_fp8(S, E, D, Fh, mode):
    # slab kernel below 1024 rows, then the two grouped tiled GEMMs (host-only query of the one plan the operator runs)
    form = ops._lib.load().m3_moe_expert_ffn_kernel(5, 0, S, E, D, Fh, None, None)
    assert form == (b"gemm_bf16w_tiled_kernel<grouped,fp8>" if S >= 1024 else b"expert_ffn_w8_kernel")
    g, x, (w1, b1, w2, b2), (q1, s1, q2, s2) = _expert_case(S, E, D, Fh, mode)
    y = ops.moe_expert_ffn(dev(x), dev(g), dev(q1), dev(b1), dev(q2), dev(b2), w1_scale=dev(s1), w2_scale=dev(s2))
    d1 = q1.double() * s1.double().unsqueeze(-1)             # dequantised weights
    d2 = q2.double() * s2.double().unsqueeze(-1)
    want = torch.zeros(S, D, dtype=torch.float64)
    for e in range(E):
        rows = (g == e).nonzero().flatten()
        if rows.numel():
            h = F.silu((r16(x[rows]) @ q1[e].double().t()) * s1[e].double() + b1[e].double())
            want[rows] = (r16(h) @ q2[e].double().t()) * s2[e].double() + b2[e].double()
    err = (y.cpu().double() - want).abs().max() / want.abs().max()
    assert float(err) < 1e-3, float(err)
    assert bool((y.cpu()[g < 0] == 0).all())
    # against the unquantised fp32 expert FFN: weight quantisation error
    from oracle import encoder_ref as ref
    y32, _, _ = ref.fmoe_expert(x.view(1, S, D), g.view(1, S, 1), w1, b1, w2, b2)
    assert float((y.cpu() - y32.view(S, D)).abs().max()) < 1e-1 * float(y32.abs().max())


def _q8(t):
    """round-to-nearest-even to e4m3, saturating at +-448 (the kernel: v_cvt_pk_fp8_f32 under MODE.FP16_OVFL -- the conversion
    itself saturates, tools/ubench/fp8_cvt_sat.hip), in fp64"""
    return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double()


@pytest.mark.parametrize("S,E,D,Fh,mode", [(4096, 32, 512, 1024, "uniform"), (16384, 32, 512, 1024, "uniform"),
                                           (6500, 8, 512, 1024, "with_dropped"), (9000, 64, 512, 1024, "uniform"),
                                           (40000, 32, 512, 1024, "with_dropped"), (5000, 16, 512, 2048, "all_one"),
                                           # persistent work-groups with several tiles each: F split in 2 / 4 (short piece
                                           # loops: part of the next tile's rows is fetched at the tile end), and 2 full tiles
                                           (20000, 32, 512, 1024, "uniform"), (10000, 32, 512, 1024, "uniform"),
                                           (65536, 32, 512, 1024, "uniform")])
def test_fmoe_expert_fp8_arithmetic(S, E, D, Fh, mode):
    """fp8 ARITHMETIC (m3_moe_expert_ffn_fp8a8: e4m3 weights x e4m3 activations, v_mfma_f32_32x32x16_fp8_fp8) against an
    fp64 evaluation of exactly the quantised computation it defines: rows quantised with the per-row scale amax / 448, H with
    the static scale h_scale, exact products, then the scales and biases.  Elements of X / H that land on an e4m3 rounding
    boundary may round the other way than in the fp64 evaluation (the kernel forms x * (448 / amax) and z in fp32): bound
    3e-3 of the output scale.  And within e4m3 accuracy (3 mantissa bits on both operands) of the unquantised fp32 FFN."""
    g, x, (w1, b1, w2, b2), (q1, s1, q2, s2) = _expert_case(S, E, D, Fh, mode)
    assert ops._lib.load().m3_moe_expert_ffn_fp8a8_active(S, E, D, Fh) == 1
    assert ops._lib.load().m3_moe_expert_ffn_kernel(5, 1, S, E, D, Fh, None, None) == b"expert_ffn_fused_fp8_kernel"
    # static H scale as the calibrator would set it: amax of the (unquantised) hidden activations x 1.25 / 448
    hmax = 0.0
    for e in range(E):
        rows = (g == e).nonzero().flatten()
        if rows.numel():
            hmax = max(hmax, float(F.silu(x[rows] @ w1[e].t() + b1[e]).abs().max()))
    h_scale = hmax * 1.25 / 448.0
    y = ops.moe_expert_ffn(dev(x), dev(g), dev(q1), dev(b1), dev(q2), dev(b2), w1_scale=dev(s1), w2_scale=dev(s2),
                           h_scale=h_scale)
    want = torch.zeros(S, D, dtype=torch.float64)
    for e in range(E):
        rows = (g == e).nonzero().flatten()
        if rows.numel():
            xr = x[rows]
            amax = xr.abs().amax(1, keepdim=True).clamp_min(1e-30)
            xq = _q8(xr * (448.0 / amax))                                  # fp32 product, as in the kernel
            sx = (amax * (1.0 / 448.0)).double()
            z = (xq @ q1[e].double().t()) * (s1[e].double() * sx) + b1[e].double()
            hq = _q8(F.silu(z).float() * (1.0 / h_scale))
            want[rows] = (hq @ q2[e].double().t()) * (s2[e].double() * h_scale) + b2[e].double()
    scale = float(want.abs().max())
    row_err = ((y.cpu().double() - want).abs().amax(1) / scale).numpy()
    live = (g >= 0).numpy()
    q50, q90, qmax = (float(np.quantile(row_err[live], q)) for q in (0.5, 0.9, 1.0))
    print("fp8 arithmetic S=%d E=%d F=%d: row error vs the fp64 evaluation of the quantised computation, of the output scale: "
          "median %.2e, 90 %% %.2e, max %.2e" % (S, E, Fh, q50, q90, qmax))
    # most rows agree to fp32 summation noise; a row where ONE element of H sits on an e4m3 rounding boundary (the kernel's
    # SiLU and the fp64 one differ by ~1e-6) moves by one e4m3 step of that element -- up to 32 h_scale for the largest
    # activations (3 mantissa bits) times a W2 entry: percent-level for that row, ~1 row in 50
    assert q50 < 2e-4 and q90 < 4e-3 and qmax < 4e-2, (q50, q90, qmax)
    assert bool((y.cpu()[g < 0] == 0).all())
    from oracle import encoder_ref as ref
    y32, _, _ = ref.fmoe_expert(x.view(1, S, D), g.view(1, S, 1), w1, b1, w2, b2)
    q_err = float((y.cpu() - y32.view(S, D)).abs().max()) / float(y32.abs().max())
    print("   vs the unquantised fp32 expert FFN: %.3e" % q_err)
    assert q_err < 8e-2, q_err


def test_quantize_rows_e4m3_matches_torch_conversion():
    """m3_quantize_rows_e4m3 (= what the fused fp8 kernel and the engine's router kernel do to a row): scale = amax / 448 exactly,
    bytes = torch's round-to-nearest-even e4m3 conversion of x * (448 / amax) -- bit for bit (rows with an exact tie between two
    e4m3 values aside: the kernel multiplies by the hardware reciprocal of amax, torch divides)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3000, 512, generator=g) * torch.logspace(-3, 3, 3000).view(-1, 1)
    x[17] = 0.0                                   # an all-zero row: scale floor, zeros out
    xq, sc = ops.quantize_rows_e4m3(dev(x))
    amax = x.abs().amax(1).clamp_min(1e-30)
    assert torch.equal(sc.cpu(), amax * (1.0 / 448.0))
    want = (x * (448.0 / amax).view(-1, 1)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    neq = (xq.cpu() != want)
    print("quantize_rows_e4m3: %d of %d bytes differ from torch's conversion" % (int(neq.sum()), neq.numel()))
    assert int(neq.sum()) <= neq.numel() // 20000       # reciprocal vs division: a handful of exact-boundary cases at most
    assert bool((xq.cpu()[17] == 0).all())


@pytest.mark.parametrize("S,E", [(8192, 64), (65536, 64), (20000, 32)])
def test_fmoe_expert_fp8_arithmetic_on_prequantised_rows_is_bit_identical(S, E):
    """m3_moe_expert_ffn_fp8a8_xq (the hand-over between the engine's router kernel and its fused fp8 expert kernel) against
    m3_moe_expert_ffn_fp8a8 on the fp32 rows: the same image and the same scales reach the same instructions, so every output bit
    must agree -- one work item per work-group (8192 rows) and the persistent loop with prefetched next tiles (65536).  This is the
    comparison that exposed the missing MFMA -> VALU wait states of the kernel's inline-asm MFMAs in round 4: the
    two instantiations are scheduled differently, and only the hazard made them differ."""
    D, Fh = 512, 1024
    g, x, (w1, b1, w2, b2), (q1, s1, q2, s2) = _expert_case(S, E, D, Fh, "uniform")
    assert ops._lib.load().m3_moe_expert_ffn_fp8a8_active(S, E, D, Fh) == 1
    args = (dev(g), dev(q1), dev(b1), dev(q2), dev(b2))
    kw = dict(w1_scale=dev(s1), w2_scale=dev(s2), h_scale=0.05)
    xd = dev(x)
    y0 = ops.moe_expert_ffn(xd, *args, **kw).clone()
    xq, sc = ops.quantize_rows_e4m3(xd)
    y1 = ops.moe_expert_ffn(xd, *args, xq=xq, xq_scale=sc, **kw).clone()
    y1b = ops.moe_expert_ffn(xd, *args, xq=xq, xq_scale=sc, **kw).clone()
    assert torch.equal(y0, y1), float((y0 - y1).abs().max())
    assert torch.equal(y1, y1b)


FP8_REL = 2e-2      # weight-only e4m3 (3 mantissa bits): measured 0.9-1.0e-2 teacher-forced


@pytest.mark.parametrize("name,cfg,lengths", [
    ("mid", EncoderConfig(num_blocks=3, embed_blocks=2), [206, 131, 333]),
    ("long_batch", EncoderConfig(num_blocks=2, embed_blocks=1), [400, 57, 206, 333, 120, 399, 250, 64, 380, 390, 395, 222, 111, 345]),
    # BASELINE configs[4]'s expert count (64), one utterance (slab kernel) and a long batch (grouped tiled GEMMs)
    ("e64_1x206", EncoderConfig(num_blocks=2, embed_blocks=1, num_experts=64), [206]),
    ("e64_batch", EncoderConfig(num_blocks=2, embed_blocks=1, num_experts=64), [400, 57, 206, 333, 120, 399, 250, 64, 380, 390, 395, 222, 111, 345]),
])
def test_engine_fp8_vs_fp32_oracle(name, cfg, lengths):
    w = make_weights(cfg, seed=11)
    g = torch.Generator().manual_seed(111)
    feat = torch.rand(len(lengths), max(lengths), cfg.input_dim, generator=g)
    fl = torch.tensor(lengths, dtype=torch.int32)
    cfg8 = EncoderConfig(**{**cfg.__dict__, "weight_dtype": "fp8"})
    eng = Engine.from_state_dict(cfg8, w)
    assert eng.weights["blocks.0.feed_forward.experts.w_1.weight"].dtype == torch.float8_e4m3fn
    assert eng.weights["blocks.0.feed_forward_macaron.w_2.weight"].dtype == torch.bfloat16
    out = eng(feat.cuda(), fl.view(1, -1).cuda()).cpu()
    B, Tp = out.shape[0], out.shape[1]
    forced = {"blocks.%d.gate_idx" % i: eng.rows_padded("blocks.%d.gate_idx" % i, torch.int32, fill=-1).cpu().view(B, Tp, 1).clone()
              for i in range(cfg.num_blocks)}
    free = {}
    encoder_forward(w, cfg, feat, fl, taps=free)
    want = encoder_forward(w, cfg, feat, fl, route_override=forced)
    valid = torch.arange(Tp).view(1, -1) < sub_len(fl.long()).view(-1, 1)
    err = float((out - want).abs()[valid].max()) / float(want.abs()[valid].max())
    print("fp8 %s: max |err| / max |logit| = %.3e (teacher-forced routing)" % (name, err))
    assert err < FP8_REL, err
    same = sum(int((forced[k].view(B, Tp)[valid] == free[k].view(B, Tp)[valid]).sum()) for k in forced)
    assert same >= 0.93 * int(valid.sum()) * cfg.num_blocks


def test_fp8_plan_round_trip(tmp_path):
    cfg = EncoderConfig(num_blocks=1, embed_blocks=1, weight_dtype="fp8")
    packed = pack_weights(make_weights(cfg, seed=4), cfg)
    path = str(tmp_path / "m.plan")
    save_plan(path, cfg, packed)
    cfg2, packed2, _ = load_plan(path)
    assert cfg2.weight_dtype == "fp8"
    for k, v in packed.items():
        a, b = packed2[k], v
        assert a.dtype == b.dtype
        if v.dtype in (torch.bfloat16, torch.float8_e4m3fn):
            a, b = a.view(torch.uint8), b.view(torch.uint8)
        assert torch.equal(a, b), k
    import os
    cfg16 = EncoderConfig(num_blocks=1, embed_blocks=1, weight_dtype="bf16")
    p16 = str(tmp_path / "m16.plan")
    save_plan(p16, cfg16, pack_weights(make_weights(cfg16, seed=4), cfg16))
    assert os.path.getsize(path) < 0.75 * os.path.getsize(p16)          # one MoE block here; 18 blocks: ~0.53
    feat = torch.rand(1, 206, cfg.input_dim, generator=torch.Generator().manual_seed(1)).cuda()
    fl = torch.tensor([[206]], dtype=torch.int32).cuda()
    assert torch.equal(Engine(cfg, packed)(feat, fl), Engine(cfg2, packed2)(feat, fl))


def test_ep_world1_fp8_equals_engine():
    from m3asr.ep import ExpertParallelEncoder
    cfg = EncoderConfig(num_blocks=2, embed_blocks=1, weight_dtype="fp8")
    w = make_weights(cfg, seed=4)
    feat = torch.rand(2, 120, cfg.input_dim, generator=torch.Generator().manual_seed(2)).cuda()
    fl = torch.tensor([[120, 107]], dtype=torch.int32).cuda()
    want = Engine.from_state_dict(cfg, w, packed_rows=False)(feat, fl).clone()
    ep = ExpertParallelEncoder(Engine.from_state_dict(cfg, w, packed_rows=False, ep_stages=True))
    assert torch.equal(ep.forward(feat, fl), want)


def test_engine_fp8_arithmetic_long_batch_calibrated():
    """EncoderConfig.fp8_activations: on a long batch the grouped expert FFN runs the fused fp8 kernel (e4m3 x e4m3 MFMA) with
    the calibrated per-layer H scale; against the fp32 oracle teacher-forced to the engine's routing the error stays at
    the e4m3 level (both operands 3 mantissa bits): <= 3e-2 of the largest logit; the weight-only engine is the reference
    point.  Short inputs of the same engine take the weight-only form (nothing to gain from quantising 50 rows)."""
    from m3asr.calibrate import calibrate_h_scales
    cfg = EncoderConfig(num_blocks=2, embed_blocks=1)
    w = make_weights(cfg, seed=11)
    rng = np.random.default_rng(5)
    lengths = rng.integers(200, 501, 64)
    lengths[0] = 500
    feat = torch.from_numpy(rng.random((64, 500, cfg.input_dim), dtype=np.float32))
    fl = torch.from_numpy(lengths.astype(np.int32))
    calib = [(torch.from_numpy(rng.random((8, 300, cfg.input_dim), dtype=np.float32)), torch.full((8,), 300, dtype=torch.int32))
             for _ in range(2)]
    scales = calibrate_h_scales(cfg, w, calib)
    assert len(scales) == cfg.num_blocks and all(1e-4 < v < 1.0 for v in scales)
    cfg8 = EncoderConfig(**{**cfg.__dict__, "weight_dtype": "fp8", "fp8_activations": True})
    eng = Engine.from_state_dict(cfg8, w)
    out = eng(feat.cuda(), fl.view(1, -1).cuda()).cpu()
    kernels = {s_["name"]: s_["kernel"] for s_ in eng.stage_info()}
    assert kernels["blocks.0.moe_local.expert"] == "expert_ffn_fused_fp8_kernel"
    B, Tp = out.shape[0], out.shape[1]
    forced = {"blocks.%d.gate_idx" % i: eng.rows_padded("blocks.%d.gate_idx" % i, torch.int32, fill=-1).cpu().view(B, Tp, 1).clone()
              for i in range(cfg.num_blocks)}
    want = encoder_forward(w, cfg, feat, fl, route_override=forced)
    valid = torch.arange(Tp).view(1, -1) < sub_len(fl.long()).view(-1, 1)
    err = float((out - want).abs()[valid].max()) / float(want.abs()[valid].max())
    w8 = Engine.from_state_dict(EncoderConfig(**{**cfg.__dict__, "weight_dtype": "fp8"}), w)
    out_w8 = w8(feat.cuda(), fl.view(1, -1).cuda()).cpu()
    assert {s_["name"]: s_["kernel"] for s_ in w8.stage_info()}["blocks.0.moe_local.expert"] != "expert_ffn_fused_fp8_kernel"
    err_w8 = float((out_w8 - want).abs()[valid].max()) / float(want.abs()[valid].max())
    print("fp8 arithmetic engine (B=64, 2 blocks): max |err| / max |logit| = %.3e teacher-forced (weight-only engine, free-running "
          "routing of its own, against the same reference: %.3e)" % (err, err_w8))
    assert err < 3e-2, err
    # short input, same engine: the weight-only expert kernel
    f1 = torch.rand(1, 206, cfg.input_dim, generator=torch.Generator().manual_seed(1)).cuda()
    l1 = torch.tensor([[206]], dtype=torch.int32).cuda()
    y1 = eng(f1, l1).clone()
    assert {s_["name"]: s_["kernel"] for s_ in eng.stage_info()}["blocks.0.moe_local.expert"] == "expert_ffn_w8_kernel"
    assert torch.equal(y1, w8(f1, l1))
