"""MXFP4 expert weights, host side: the quantiser of m3asr/plan.py against the float64 restatement of the format
(tests/mxfp4_ref.py), the packed layouts, the plan file, and the form the one expert-FFN plan answers for the new dtype.
No GPU is needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mxfp4_ref
from m3asr import _lib
from m3asr.config import EncoderConfig
from m3asr.plan import (EXPERT_SLICE, cast_gemm_weights, dequantize_mxfp4, load_plan, pack_weights, quantize_mxfp4, save_plan)
from m3asr.weights import make_weights

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _cases():
    rng = np.random.default_rng(7)
    out = {}
    out["gaussian"] = rng.standard_normal((16, 64)).astype(np.float32) * np.logspace(-3, 3, 16, dtype=np.float32)[:, None]
    # exact grid values, both signs, at several block exponents (the block's largest magnitude is 4 or 6: scale = 2^e exactly)
    rows = []
    for e in (-20, -3, 0, 5, 17):
        v = np.array([GRID[i % 8] * (-1) ** (i // 8) for i in range(32)]) * 2.0 ** e
        rows.append(np.concatenate([v, v[::-1]]))
    out["grid"] = np.array(rows, dtype=np.float32)
    # exact ties between neighbouring grid values (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5) next to a 4.0 that pins the scale at 1
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    v = np.array([4.0] + ties + [-t for t in ties] + [0.0] * 17)
    out["ties"] = np.stack([np.concatenate([v, v * 2.0 ** -9]), np.concatenate([v * 8.0, v[::-1]])]).astype(np.float32)
    o = rng.standard_normal((4, 64)).astype(np.float32) * 0.01
    o[:, 5] = 37.0                                  # one outlier: everything else in its block rounds to 0 / 0.5 steps of 8
    o[2, 40] = -1000.0
    out["outlier"] = o
    z = rng.standard_normal((2, 64)).astype(np.float32)
    z[0, :32] = 0.0                                 # an all-zero block
    z[1, 32:] = 0.0
    out["zero_block"] = z
    t = np.zeros((2, 64), dtype=np.float32)
    t[0, :32] = (2.0 ** -80) * np.where(np.arange(32) % 3 == 0, -1.0, 1.0)     # amax 2^-80: below the clamp, zero codes
    t[1, 3] = 2.0 ** -80
    out["tiny"] = t
    s = np.ones((3, 32), dtype=np.float32)
    s[0, 0], s[0, 1] = 7.9, -7.5                    # amax in (6, 8): scale 1, the values saturate at +-6
    s[1, :4] = [15.9, 13.0, -12.1, 10.1]
    s[2, :] = 2.0 ** 100 * np.linspace(0.8, 1.99, 32)   # beyond the scale clamp (e = 64): saturates
    out["saturate"] = s
    return out


@pytest.mark.parametrize("name", ["gaussian", "grid", "ties", "outlier", "zero_block", "tiny", "saturate"])
def test_quantize_mxfp4_equals_restatement(name):
    w = _cases()[name]
    q, s = quantize_mxfp4(torch.from_numpy(w), dim=1)
    q_ref, s_ref = mxfp4_ref.quantize(w)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert tuple(q.shape) == (w.shape[0], w.shape[1] // 2) and tuple(s.shape) == (w.shape[0], w.shape[1] // 32)
    assert np.array_equal(s.numpy(), s_ref), (s.numpy(), s_ref)
    assert np.array_equal(q.numpy(), q_ref), np.argwhere(q.numpy() != q_ref)[:4]
    assert int(s.min()) >= 63 and int(s.max()) <= 191
    assert np.array_equal(dequantize_mxfp4(q, s, dim=1).double().numpy(), mxfp4_ref.decode(q_ref, s_ref))
    if name == "tiny":
        assert int(q.max()) == 0 and set(s.flatten().tolist()) <= {63, 127}
    if name == "zero_block":
        assert int(s[0, 0]) == 127 and int(s[1, 1]) == 127 and int(q[0, :16].max()) == 0
    if name == "saturate":
        d = dequantize_mxfp4(q, s, dim=1)
        assert d[0, 0] == 6.0 and d[0, 1] == -6.0 and int(s[2, 0]) == 191 and float(d[2].max()) == 6.0 * 2.0 ** 64
    if name == "ties":
        d = dequantize_mxfp4(q, s, dim=1)[0, :8].tolist()
        assert d == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0], d       # every tie went to the even code


def test_decode_inverts_on_grid_values_and_other_axes():
    w = torch.from_numpy(_cases()["grid"])
    q, s = quantize_mxfp4(w, dim=1)
    assert torch.equal(dequantize_mxfp4(q, s, dim=1), w)
    # blocks along a middle axis: the same codes as along the last axis of the transposed tensor
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3, 64, 5, generator=g)
    q1, s1 = quantize_mxfp4(t, dim=1)
    q2, s2 = quantize_mxfp4(t.transpose(1, 2).contiguous(), dim=2)
    assert torch.equal(q1, q2.transpose(1, 2)) and torch.equal(s1, s2.transpose(1, 2))
    d = dequantize_mxfp4(q1, s1, dim=1)
    assert d.shape == t.shape
    # requantising decoded values changes nothing (they are on the grid of their own scale)
    q3, s3 = quantize_mxfp4(d, dim=1)
    assert torch.equal(dequantize_mxfp4(q3, s3, dim=1), d)
    with pytest.raises(AssertionError):
        quantize_mxfp4(torch.zeros(4, 48), dim=1)


def test_cast_gemm_weights_mxfp4_shapes_and_dense_tensors():
    cfg4 = EncoderConfig(num_blocks=1, embed_blocks=1, weight_dtype="mxfp4")
    cfg8 = EncoderConfig(num_blocks=1, embed_blocks=1, weight_dtype="fp8")
    cfg32 = EncoderConfig(num_blocks=1, embed_blocks=1)
    w = make_weights(cfg32, seed=4)
    p32, p4, p8 = pack_weights(w, cfg32), pack_weights(w, cfg4), pack_weights(w, cfg8)
    E, F, D = cfg4.num_experts, cfg4.hidden_units, cfg4.attention_dim
    f = "blocks.0.feed_forward.experts."
    want = {f + "w_1.weight": (E, F, D // 2), f + "w_1.scale": (E, F, D // 32),
            f + "w_2.weight_sliced": (E, F // EXPERT_SLICE, D, EXPERT_SLICE // 2), f + "w_2.scale": (E, F // EXPERT_SLICE, D, 2)}
    for k, shape in want.items():
        assert p4[k].dtype == torch.uint8 and tuple(p4[k].shape) == shape, (k, p4[k].dtype, tuple(p4[k].shape))
    assert set(p4) == set(p8)
    for k in p4:
        if k not in want:                              # everything that is not an expert weight: exactly what the fp8 mode stores
            assert p4[k].dtype == p8[k].dtype and torch.equal(p4[k].view(torch.uint8), p8[k].view(torch.uint8)), k
    # the stored codes are the quantiser's, along each GEMM's K, and decode to within the format's step of the fp32 weights
    q, s = quantize_mxfp4(p32[f + "w_1.weight"], dim=2)
    assert torch.equal(q, p4[f + "w_1.weight"]) and torch.equal(s, p4[f + "w_1.scale"])
    d2 = dequantize_mxfp4(p4[f + "w_2.weight_sliced"], p4[f + "w_2.scale"], dim=3)
    w2 = p32[f + "w_2.weight_sliced"]
    step = torch.ldexp(torch.ones(()), p4[f + "w_2.scale"].to(torch.int32) - 127).repeat_interleave(32, -1)
    # half the coarsest grid step (2 scale units), or up to 2 units where a block's largest value in (6, 8) saturates at 6
    assert bool(((d2 - w2).abs() <= 2 * step).all())
    rms = float((d2 - w2).pow(2).mean().sqrt() / w2.pow(2).mean().sqrt())
    print("mxfp4 rms weight error %.3f" % rms)
    assert 0.05 < rms < 0.25
    # a no-op on weights that are not fp32 any more
    again = cast_gemm_weights(p4, cfg4)
    assert all(torch.equal(again[k].view(torch.uint8), p4[k].view(torch.uint8)) for k in p4)


def test_mxfp4_plan_round_trip_and_size(tmp_path):
    cfg = EncoderConfig(num_blocks=1, embed_blocks=1, weight_dtype="mxfp4")
    packed = pack_weights(make_weights(cfg, seed=4), cfg)
    path = str(tmp_path / "m4.plan")
    save_plan(path, cfg, packed)
    cfg2, packed2, _ = load_plan(path)
    assert cfg2.weight_dtype == "mxfp4" and list(packed2) == list(packed)
    for k, v in packed.items():
        assert packed2[k].dtype == v.dtype and tuple(packed2[k].shape) == tuple(v.shape), k
        assert torch.equal(packed2[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    cfg8 = EncoderConfig(num_blocks=1, embed_blocks=1, weight_dtype="fp8")
    p8 = str(tmp_path / "m8.plan")
    save_plan(p8, cfg8, pack_weights(make_weights(cfg8, seed=4), cfg8))
    n4, n8 = os.path.getsize(path), os.path.getsize(p8)
    print("plan bytes, one MoE block: mxfp4 %d, fp8 %d" % (n4, n8))
    E, F, D = cfg.num_experts, cfg.hidden_units, cfg.attention_dim
    # per expert GEMM pair: 2 D F bytes (fp8) -> D F codes + D F / 16 scale bytes; the fp8 row scales (4 (F + D) per expert) go
    assert n4 < n8 and abs((n8 - n4) - E * (2 * D * F - D * F - D * F // 16 + 4 * (F + D))) <= 4 * 256


def test_config_rejects_fp8_activations_with_mxfp4():
    with pytest.raises(ValueError, match="mxfp4"):
        EncoderConfig(weight_dtype="mxfp4", fp8_activations=True)


def test_expert_plan_answers_the_w4_forms():
    """m3_moe_expert_ffn_kernel(M3_MXFP4 = 6, ...): the slab kernel below M3_EXPERT_TILED_MIN_ROWS (1024), the grouped tiled GEMM
    from it on; D must be a multiple of 128 for the slab form (192: none), of 128 as well for the tiled one."""
    lib = _lib.load()
    assert _lib.MXFP4 == 6

    def ask(S, E, D, F, act=0):
        launches, slices = C.c_int32(-1), C.c_int32(-1)
        label = lib.m3_moe_expert_ffn_kernel(6, act, S, E, D, F, C.byref(launches), C.byref(slices))
        return (label.decode() if label else None), launches.value, slices.value

    assert ask(50, 32, 512, 1024) == ("expert_ffn_w4_kernel", 1, 16)
    assert ask(1023, 32, 512, 1024) == ("expert_ffn_w4_kernel", 1, 16)
    assert ask(1024, 32, 512, 1024) == ("gemm_bf16w_tiled_kernel<grouped,mxfp4>", 2, 1)
    assert ask(2048, 8, 128, 256) == ("gemm_bf16w_tiled_kernel<grouped,mxfp4>", 2, 1)
    assert ask(5000, 32, 512, 1088) == ("expert_ffn_w4_kernel", 1, 17)       # F a multiple of 64 but not of 128: slabs
    assert ask(50, 8, 192, 256)[0] is None                                    # D not a multiple of 128: no form
    assert ask(50, 8, 64, 256)[0] is None
    assert ask(50, 32, 512, 1024, act=1)[0] is None                           # no fp8 arithmetic on 4-bit weights
