"""MXFP4 expert weights (W4A16) on the GPU.

The weights are decoded to bf16 at the MFMA input, exactly (an e2m1 value times a power of two is a bf16 number), so the
arithmetic is that of the bf16 kernels on the decoded weights and kernel error separates from quantisation error.  Levels:
  * every e2m1 code, at several block scales, through the slab kernel itself: pins nibble, byte and block order of the decode;
  * the operator (slab form and the two grouped tiled GEMMs) against a float64 evaluation on the decoded weights
    (tests/mxfp4_ref.py decodes; x and H rounded to bf16 as the kernels round them), bound 1e-3 of the largest output;
  * one slab case on a strided x with every operand between guards;
  * the whole encoder against the CPU oracle GIVEN the decoded expert weights, routing teacher-forced: the bf16 bound;
    against the fp32 weights the error is printed only (it is the cost of the format: DESIGN.md 30);
  * plan round trip and chunked streaming identity; what engine creation refuses.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded as G
import mxfp4_ref
from m3asr import _lib, ops
from m3asr.config import EncoderConfig, subsampled_len
from m3asr.engine import Engine
from m3asr.plan import dequantize_mxfp4, load_plan, pack_weights, quantize_mxfp4, save_plan
from m3asr.weights import make_weights
from oracle.encoder_ref import encoder_forward, sub_len

BF16_REL = 2e-2     # the project's bound for bf16 arithmetic against the fp32 oracle (tests/test_bf16_gpu.py)


def dev(t):
    return t.cuda().contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r16(t):
    return t.float().to(torch.bfloat16).double()


def _form(S, E, D, Fh):
    return ops._lib.load().m3_moe_expert_ffn_kernel(6, 0, S, E, D, Fh, None, None)


def test_every_e2m1_code_through_the_kernel():
    """One expert, D = 128, F = 64.  Row 0 of W1 holds the 16 codes repeated, its four blocks carry the scale codes 120, 127,
    130, 127; the rows of x are one-hot; W2 is the identity on hidden unit 0.  Output column 0 is SiLU of the decoded W1 row.
    Neighbouring e2m1 values are >= 20 % apart and the blocks differ by factors of 8 and 128: a swapped nibble, byte, dword or
    block puts a value at a wrong k and shows."""
    E, D, Fh = 1, 128, 64
    codes = np.arange(D) % 16
    q1 = np.zeros((E, Fh, D // 2), dtype=np.uint8)
    q1[0, 0] = codes[0::2] | (codes[1::2] << 4)
    s1 = np.full((E, Fh, D // 32), 127, dtype=np.uint8)
    s1[0, 0] = [120, 127, 130, 127]
    q2 = np.zeros((E, D, Fh // 2), dtype=np.uint8)
    q2[0, 0, 0] = 2                                           # k = 0: code 2 = 1.0, k = 1: 0
    s2 = np.full((E, D, Fh // 32), 127, dtype=np.uint8)
    assert mxfp4_ref.decode(q2, s2)[0, 0, 0] == 1.0 and mxfp4_ref.decode(q2, s2).sum() == 1.0
    x = torch.eye(D)
    g = torch.zeros(D, dtype=torch.int32)
    assert _form(D, E, D, Fh) == b"expert_ffn_w4_kernel"
    y = ops.moe_expert_ffn(dev(x), dev(g), dev(torch.from_numpy(q1)), torch.zeros(E, Fh).cuda(), dev(torch.from_numpy(q2)),
                           torch.zeros(E, D).cuda(), w1_scale=dev(torch.from_numpy(s1)), w2_scale=dev(torch.from_numpy(s2))).cpu()
    vals = torch.from_numpy(mxfp4_ref.decode(q1, s1)[0, 0])
    assert len(set(vals.tolist())) >= 40                      # 15 distinct values x 3 scales (+-0 once)
    want = F.silu(vals).float()
    # H passes through bf16 and a fast-math SiLU: the tolerance of test_device_e4m3_decoding_matches_torch
    assert torch.allclose(y[:, 0], want, rtol=2 ** -7, atol=1e-6), (y[:, 0] - want).abs().max().item()
    assert bool((y[:, 1:] == 0).all())


def _expert_case(S, E, D, Fh, mode):
    rng = np.random.default_rng(S + E)
    g = {"uniform": rng.integers(0, E, S), "all_one": np.full(S, 3 % E), "with_dropped": rng.integers(-1, E, S)}[mode]
    g = torch.from_numpy(g.astype(np.int32))
    x = rnd(S, D, seed=1)
    w1, b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
    w2, b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
    q1, s1 = quantize_mxfp4(w1, dim=2)
    q2, s2 = quantize_mxfp4(w2, dim=2)
    return g, x, (w1, b1, w2, b2), (q1, s1, q2, s2)


def _want(g, x, b1, b2, q, E):
    q1, s1, q2, s2 = q
    d1 = torch.from_numpy(mxfp4_ref.decode(q1.numpy(), s1.numpy()))        # float64, the restatement's decode
    d2 = torch.from_numpy(mxfp4_ref.decode(q2.numpy(), s2.numpy()))
    want = torch.zeros(x.shape[0], x.shape[1], dtype=torch.float64)
    for e in range(E):
        rows = (g == e).nonzero().flatten()
        if rows.numel():
            h = F.silu(r16(x[rows]) @ d1[e].t() + b1[e].double())
            want[rows] = r16(h) @ d2[e].t() + b2[e].double()
    return want


@pytest.mark.parametrize("S,E,D,Fh,mode,form", [
    (37, 4, 128, 128, "with_dropped", "slab"),        # two slices, partial row tile
    (50, 32, 512, 1024, "uniform", "slab"),           # the served dimensions; experts with no rows
    (200, 8, 256, 128, "all_one", "slab"),            # MT = 2; D / 128 = 2 steps
    (1090, 8, 128, 256, "with_dropped", "tiled"),     # ragged last tile; rows with index < 0 give exact zeros
    (2048, 32, 512, 1024, "uniform", "tiled"),        # served dimensions at tiled row count
])
def test_fmoe_expert_mxfp4(S, E, D, Fh, mode, form):
    assert _form(S, E, D, Fh) == {"slab": b"expert_ffn_w4_kernel", "tiled": b"gemm_bf16w_tiled_kernel<grouped,mxfp4>"}[form]
    g, x, (w1, b1, w2, b2), q = _expert_case(S, E, D, Fh, mode)
    q1, s1, q2, s2 = q
    y = ops.moe_expert_ffn(dev(x), dev(g), dev(q1), dev(b1), dev(q2), dev(b2), w1_scale=dev(s1), w2_scale=dev(s2)).cpu()
    want = _want(g, x, b1, b2, q, E)
    err = float((y.double() - want).abs().max() / want.abs().max())
    print("mxfp4 expert FFN S=%d E=%d D=%d F=%d (%s): max |err| / max |y| = %.3e against float64 on the decoded weights" % (S, E, D, Fh, form, err))
    assert err < 1e-3, err
    assert bool((y[g < 0] == 0).all())


def test_fmoe_expert_mxfp4_strided_guarded():
    """m3_moe_expert_ffn_mxfp4_ldx on x with ldx > D, every operand between guards (tests/guarded.py): NaN around the float
    inputs, saturated codes and a 2^23 scale around the weight bytes, -1 (a dropped row) around gate_idx; the output's guards
    must come back untouched and the values must be those of the dense call."""
    S, E, D, Fh = 37, 4, 128, 128
    assert _form(S, E, D, Fh) == b"expert_ffn_w4_kernel"
    g, x, (w1, b1, w2, b2), q = _expert_case(S, E, D, Fh, "with_dropped")
    q1, s1, q2, s2 = q
    lib = _lib.load()
    gx = G.strided_in(x)
    assert gx.ld > D
    gg = G.flat_in(g, int_guard=-1)
    gq1, gq2 = G.flat_in(q1, int_guard=0x77), G.flat_in(q2, int_guard=0x77)
    gs1, gs2 = G.flat_in(s1, int_guard=150), G.flat_in(s2, int_guard=150)
    gb1, gb2 = G.flat_in(b1), G.flat_in(b2)
    gy = G.flat_out((S, D))
    ws = torch.empty(ops.moe_expert_workspace_size(S, E, D, Fh), dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.m3_moe_expert_ffn_mxfp4_ldx(P(gx.view), gx.ld, P(gg.view), P(gq1.view), P(gs1.view), P(gb1.view), P(gq2.view),
                                         P(gs2.view), P(gb2.view), S, E, D, Fh, None, None, 1.0, None, None, 0.0, P(gy.view),
                                         P(ws), ws.numel(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    gy.check("mxfp4 expert FFN y")
    y = gy.view.cpu()
    want = _want(g, x, b1, b2, q, E)
    assert float((y.double() - want).abs().max() / want.abs().max()) < 1e-3
    dense = ops.moe_expert_ffn(dev(x), dev(g), dev(q1), dev(b1), dev(q2), dev(b2), w1_scale=dev(s1), w2_scale=dev(s2)).cpu()
    assert torch.equal(y, dense)
    # a stride shorter than a row, or not a multiple of 4, is refused
    for bad in (D - 4, D + 2):
        assert lib.m3_moe_expert_ffn_mxfp4_ldx(P(gx.view), bad, P(gg.view), P(gq1.view), P(gs1.view), P(gb1.view), P(gq2.view),
                                               P(gs2.view), P(gb2.view), S, E, D, Fh, None, None, 1.0, None, None, 0.0,
                                               P(gy.view), P(ws), ws.numel(), None) != 0


def _decoded_expert_weights(w, cfg):
    """the reference-layout weights with every expert matrix replaced by what the mxfp4 plan stores for it, decoded
    (blocks along each GEMM's K: D for w_1 [E,F,D], F for w_2 [E,D,F] -- a 64-wide slice of the plan is two such blocks)"""
    out = dict(w)
    for i in range(cfg.num_blocks):
        for n in ("w_1", "w_2"):
            k = "blocks.%d.feed_forward.experts.%s.weight" % (i, n)
            out[k] = dequantize_mxfp4(*quantize_mxfp4(w[k].float(), dim=2), dim=2)
    return out


@pytest.mark.parametrize("lengths", [[206], [206, 131, 333]])
def test_engine_mxfp4_vs_decoded_weight_oracle(lengths):
    base = EncoderConfig(num_blocks=2, embed_blocks=1)
    cfg4 = EncoderConfig(num_blocks=2, embed_blocks=1, weight_dtype="mxfp4")
    w = make_weights(base, seed=11)
    wd = _decoded_expert_weights(w, base)
    g = torch.Generator().manual_seed(111)
    feat = torch.rand(len(lengths), max(lengths), base.input_dim, generator=g)
    fl = torch.tensor(lengths, dtype=torch.int32)
    eng = Engine.from_state_dict(cfg4, w)
    assert eng.weights["blocks.0.feed_forward.experts.w_1.weight"].dtype == torch.uint8
    assert eng.weights["blocks.0.feed_forward.experts.w_2.scale"].dtype == torch.uint8
    assert eng.weights["blocks.0.feed_forward_macaron.w_2.weight"].dtype == torch.bfloat16
    out = eng(feat.cuda(), fl.view(1, -1).cuda()).cpu()
    kernels = {s_["name"]: s_["kernel"] for s_ in eng.stage_info()}
    assert kernels["blocks.0.moe_local.expert"] == "expert_ffn_w4_kernel"
    B, Tp = out.shape[0], out.shape[1]
    forced = {"blocks.%d.gate_idx" % i: eng.rows_padded("blocks.%d.gate_idx" % i, torch.int32, fill=-1).cpu().view(B, Tp, 1).clone()
              for i in range(base.num_blocks)}
    free = {}
    encoder_forward(wd, base, feat, fl, taps=free)
    want = encoder_forward(wd, base, feat, fl, route_override=forced)
    valid = torch.arange(Tp).view(1, -1) < sub_len(fl.long()).view(-1, 1)
    err = float((out - want).abs()[valid].max()) / float(want.abs()[valid].max())
    want32 = encoder_forward(w, base, feat, fl, route_override=forced)
    err32 = float((out - want32).abs()[valid].max()) / float(want32.abs()[valid].max())
    same = sum(int((forced[k].view(B, Tp)[valid] == free[k].view(B, Tp)[valid]).sum()) for k in forced)
    share = same / float(int(valid.sum()) * base.num_blocks)
    print("mxfp4 %s: max |err| / max |logit| = %.3e against the oracle on the decoded expert weights, %.3e against the fp32 "
          "weights (teacher-forced routing); routing agreement with the decoded-weight oracle %.4f" % (lengths, err, err32, share))
    assert err < BF16_REL, err
    assert share >= 0.93, share


def test_mxfp4_plan_round_trip_engine_identity(tmp_path):
    cfg = EncoderConfig(num_blocks=2, embed_blocks=1, weight_dtype="mxfp4")
    packed = pack_weights(make_weights(cfg, seed=4), cfg)
    path = str(tmp_path / "m4.plan")
    save_plan(path, cfg, packed)
    cfg2, packed2, _ = load_plan(path)
    feat = torch.rand(1, 206, cfg.input_dim, generator=torch.Generator().manual_seed(1)).cuda()
    fl = torch.tensor([[206]], dtype=torch.int32).cuda()
    assert torch.equal(Engine(cfg, packed)(feat, fl), Engine(cfg2, packed2)(feat, fl))


def test_mxfp4_chunked_streaming_matches_full_forward():
    """One 206-frame utterance through the causal model, chunk by chunk, against the full forward: the comparison and the
    tolerance of test_chunked_bf16_within_16bit_bound (the two run GEMM kernels of different shapes; a router near-tie may
    fall the other way, and the model being causal only frames from that chunk on can differ)."""
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=16,
                        num_decoding_left_chunks=3, weight_dtype="mxfp4")
    w = make_weights(cfg, seed=33)
    g = torch.Generator().manual_seed(6)
    feat, fl = torch.rand(1, 206, cfg.input_dim, generator=g), torch.tensor([206], dtype=torch.int32)
    eng = Engine.from_state_dict(cfg, w, packed_rows=False, bf16_activations=False)
    full = eng(feat.cuda().contiguous(), fl.view(1, -1).cuda().contiguous()).cpu()
    Tp = full.shape[1]
    full_gi = torch.stack([eng.buffer("blocks.%d.gate_idx" % i, torch.int32).view(1, Tp).clone() for i in range(cfg.num_blocks)]).cpu()
    st = eng.streaming(1, Tp)
    c = st.c
    n_chunks = -(-Tp // c)
    padded = torch.zeros(1, max(206, 4 * c * n_chunks + 3), feat.shape[2])
    padded[:, :206] = feat
    st.reset()
    outs, gates = [], []
    for n in range(n_chunks):
        left = (fl.long() - 4 * c * n).clamp(min=0, max=st.window)
        left = torch.where(left >= 7, left, torch.zeros_like(left))
        lg = st.step(padded[:, 4 * c * n: 4 * c * n + st.window], left)
        eng.stream.synchronize()
        outs.append(lg.clone())
        gates.append(torch.stack([st.buffer("blocks.%d.gate_idx" % i, torch.int32).view(1, c).clone() for i in range(cfg.num_blocks)]))
    got, gi = torch.cat(outs, 1)[:, :Tp].cpu(), torch.cat(gates, 2)[:, :, :Tp].cpu()
    assert Tp == subsampled_len(206)
    differs = (gi != full_gi).any(dim=0).view(-1)
    agree = float((gi == full_gi).float().mean())
    upto = (int(differs.nonzero()[0]) // c) * c if bool(differs.any()) else Tp     # causal: chunks before the first flip
    rel = float((got - full)[:, :upto].abs().max()) / float(full.abs().max()) if upto else 0.0
    print("mxfp4 chunked vs full forward: max |diff| / max |logit| = %.3e on the first %d of %d frames, routing agreement %.5f"
          % (rel, upto, Tp, agree))
    assert agree >= 0.995, agree
    assert rel <= 1e-2, rel


def test_engine_create_rejects_what_mxfp4_does_not_support():
    base = dict(num_blocks=1, embed_blocks=1)
    with pytest.raises(ValueError, match="fp8_activations"):
        EncoderConfig(weight_dtype="mxfp4", fp8_activations=True, **base)
    # the C entry refuses it too (a caller that fills m3_engine_config itself)
    cfg = EncoderConfig(weight_dtype="mxfp4", **base)
    packed = pack_weights(make_weights(cfg, seed=4), cfg)
    import m3asr.engine as me
    orig = me._engine_config

    def forced(c, *a, **k):
        ec = orig(c, *a, **k)
        ec.fp8_activations = 1
        return ec
    me._engine_config = forced
    try:
        with pytest.raises(_lib.M3Error, match="fp8_activations"):
            Engine(cfg, packed)
    finally:
        me._engine_config = orig
    # expert parallelism is out of scope for this mode
    cfg_ep = EncoderConfig(weight_dtype="mxfp4", ep_world_size=2, ep_rank=0, num_experts=16, **base)
    w_ep = make_weights(EncoderConfig(num_experts=32, **base), seed=4)
    with pytest.raises(_lib.M3Error, match="expert parallelism"):
        Engine.from_state_dict(cfg_ep, w_ep)
    # attention_dim = 192: a multiple of 64 (what fp8 needs) but not of 128
    cfg192 = EncoderConfig(weight_dtype="mxfp4", attention_dim=192, embed_dim=192, attention_heads=4, embed_heads=4, **base)
    with pytest.raises(_lib.M3Error, match="multiple of 128"):
        Engine.from_state_dict(cfg192, make_weights(cfg192, seed=4))


def test_builder_mxfp4_flag_writes_an_mxfp4_plan_that_infer_runs(tmp_path):
    """synthetic checkpoint -> builder.py --mxfp4 -> infer.py; --mxfp4 together with another precision flag is refused"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "3m-asr-inference_amd"))
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "make_synthetic_checkpoint.py"), "--out-dir", d,
                           "--layers", "1", "--seed", "3"], env=env)
    plan = os.path.join(d, "enc4.plan")
    common = [sys.executable, os.path.join(root, "builder.py"), "-c", os.path.join(d, "config.yaml"), "-m",
              os.path.join(d, "model.pt"), "-o", plan, "--opt-shape", "2x64"]
    out = subprocess.check_output(common + ["--mxfp4"], env=env, text=True)
    assert "fused engine vs op-by-op emission" in out
    cfg4, packed4, _ = load_plan(plan)
    assert cfg4.weight_dtype == "mxfp4"
    assert packed4["blocks.0.feed_forward.experts.w_1.weight"].dtype == torch.uint8
    assert packed4["blocks.0.feed_forward.experts.w_2.scale"].dtype == torch.uint8
    assert packed4["blocks.0.feed_forward_macaron.w_2.weight"].dtype == torch.bfloat16
    np.save(os.path.join(d, "feat.npy"), np.random.default_rng(0).random((1, 206, 40), dtype=np.float32))
    out = subprocess.check_output([sys.executable, os.path.join(root, "infer.py"), "-p", plan, "-i", os.path.join(d, "feat.npy")],
                                  env=env, text=True)
    assert "time=" in out and "outputs.shape:(1, 50," in out
    r = subprocess.run(common + ["--mxfp4", "--fp8"], env=env, text=True, capture_output=True)
    assert r.returncode != 0 and "mutually exclusive" in r.stderr
