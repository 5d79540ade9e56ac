"""Fragment-ordered fp32 weights (include/m3asr.h "fragment order"), the host side: the packers, the planner's
answer for a descriptor whose w is in that order (m3_linear_wfrag_kernel), and what must not move -- the bytes of a saved plan
and of a serialised config.  No GPU.

The layout is written out here once more, as the literal index formula, on purpose: the packers are checked against it and
not against each other alone.

Refused cases go through m3_linear_wfrag_kernel and m3_linear_wfrag (which refuses on the host, before any HIP call).  The
implicit conv has no entry that takes fragment-ordered weights (m3_conv2d_3x3s2 never sets the flag), so its refusal is not
reachable from the boundary; the concat refusal stands for "not plain A"."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from m3asr import _lib
from m3asr.config import EncoderConfig
from m3asr.plan import (EXPERT_SLICE, add_frag_weights, pack_weights, pack_wfrag, save_plan, slice_major_w2, unpack_wfrag)
from m3asr.weights import make_weights
from test_gemm_plan_host import desc, row

SKINNY = "gemm_f32_kernel"


def distinct(*shape):
    n = int(np.prod(shape))
    return torch.arange(n, dtype=torch.float32).reshape(*shape)


def test_packer_is_the_index_formula():
    N, K = 32, 48
    w = distinct(N, K)
    wf = pack_wfrag(w)
    assert tuple(wf.shape) == (N // 16, K // 16, 4, 16, 4) and wf.is_contiguous()
    want = torch.empty_like(wf)
    for nt in range(N // 16):
        for s in range(K // 16):
            for kq in range(4):
                for col in range(16):
                    for j in range(4):
                        want[nt, s, kq, col, j] = w[16 * nt + col, 16 * s + 4 * kq + j]
    assert torch.equal(wf, want)
    # lane l = 16 kq + col reads bytes [16 l, 16 l + 16) of the KB of (nt, s): the four floats W[16 nt + col][16 s + 4 kq ..]
    flat = wf.reshape(N // 16, K // 16, 64, 4)
    for lane in (0, 1, 15, 16, 37, 63):
        col, kq = lane & 15, lane >> 4
        assert torch.equal(flat[1, 2, lane], w[16 + col, 32 + 4 * kq: 32 + 4 * kq + 4])


def test_pack_unpack_identity():
    g = torch.Generator().manual_seed(1)
    dense = torch.randn(48, 80, generator=g)
    assert torch.equal(unpack_wfrag(pack_wfrag(dense)), dense)
    E, F, D = 3, 2 * EXPERT_SLICE, 48
    w1 = torch.randn(E, F, D, generator=g)
    f1 = pack_wfrag(w1)
    assert tuple(f1.shape) == (E, F // 16, D // 16, 4, 16, 4)
    assert torch.equal(unpack_wfrag(f1), w1)
    for e in range(E):      # per expert: the dense layout with N = F, K = D
        assert torch.equal(f1[e], pack_wfrag(w1[e]))
    w2 = torch.randn(E, D, F, generator=g)
    s2 = slice_major_w2(w2)
    f2 = pack_wfrag(s2)
    assert tuple(f2.shape) == (E, F // EXPERT_SLICE, D // 16, EXPERT_SLICE // 16, 4, 16, 4)
    assert torch.equal(unpack_wfrag(f2), s2)
    # f2[e][sl][sub][st][kq][col][j] = w2[e][16 sub + col][64 sl + 16 st + 4 kq + j]
    for (e, sl, sub, st, kq, col, j) in [(0, 0, 0, 0, 0, 0, 0), (2, 1, 2, 3, 1, 7, 2), (1, 0, 1, 2, 3, 15, 3)]:
        assert f2[e, sl, sub, st, kq, col, j] == w2[e, 16 * sub + col, EXPERT_SLICE * sl + 16 * st + 4 * kq + j]


@pytest.mark.parametrize("N,K", [(16, 16), (32, 48), (48, 80)])
def test_python_and_c_packers_agree(N, K):
    lib = _lib.load()
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)).numpy()
    out = np.full(N * K, np.nan, dtype=np.float32)
    assert lib.m3_pack_wfrag_host(w.ctypes.data, N, K, out.ctypes.data) == 0
    assert out.tobytes() == pack_wfrag(torch.from_numpy(w)).numpy().tobytes()
    assert lib.m3_pack_wfrag_host(w.ctypes.data, 40, K, out.ctypes.data) != 0
    assert _lib.last_error() == "pack_wfrag: N=40 and K=%d must be positive multiples of 16" % K


ACCEPTED = [row(50, 1024, 512), row(50, 96, 512, act="glu"), row(1, 16, 16), row(50, 2048, 512, act="glu", ln="folded", mask_in=True), row(50, 512, 2048, resid=True),
            row(17, 48, 80, act="silu"), row(383, 2048, 512), row(640, 1024, 512, ln="affine")]
REFUSED = [
    (row(50, 40, 512), "gemm: fragment-ordered weights need N=40 and K=512 to be multiples of 16"),
    (row(50, 1024, 24), "gemm: K=24 must be a multiple of 16"),
    (row(50, 1024, 768, k1=256), "gemm: fragment-ordered weights need plain A (no concat, no implicit conv)"),
    (row(50, 1024, 512, w="bf16"), "gemm: fragment-ordered weights are fp32-only"),
    (row(640, 1024, 512), "gemm: fragment-ordered weights need the skinny fp32 kernel; M=640 N=1024 K=512 plans as gemm_f32_tiled_kernel"),
    (row(50, 80, 512, act="glu"), "gemm: fragment-ordered weights need N / 2=40 and K=512 to be multiples of 16"),
]


@pytest.mark.parametrize("r", ACCEPTED, ids=lambda r: "%dx%dx%d-%s" % (r["M"], r["N"], r["K"], r["act"]))
def test_plan_accepts(r):
    lib = _lib.load()
    d = desc(r)
    name = lib.m3_linear_wfrag_kernel(C.byref(d))
    assert name is not None and name.decode() == SKINNY, _lib.last_error()
    assert lib.m3_linear_kernel(C.byref(d), 0).decode() == SKINNY      # the same form as without the flag


@pytest.mark.parametrize("r,msg", REFUSED, ids=[m.split(": ")[1][:40].replace(" ", "_") + "-%dx%dx%d" % (r["M"], r["N"], r["K"]) for r, m in REFUSED])
def test_plan_refuses(r, msg):
    lib = _lib.load()
    d = desc(r)
    assert lib.m3_linear_wfrag_kernel(C.byref(d)) is None
    assert _lib.last_error() == msg
    assert lib.m3_linear_wfrag(C.byref(d), None) != 0      # refused by the plan on the host, before any HIP call
    assert _lib.last_error() == msg


def small_cfg(**kw):
    return EncoderConfig(output_dim=32, attention_dim=256, attention_heads=4, num_blocks=2, embed_heads=4, embed_dim=256,
                         embed_linear_units=256, embed_blocks=1, num_experts=8, hidden_units=64, **kw)


def plan_bytes(cfg, packed, tmp_path, name):
    path = tmp_path / name
    save_plan(str(path), cfg, packed)
    return path.read_bytes()


def test_save_plan_does_not_see_the_fragment_tensors(tmp_path):
    cfg = small_cfg()
    packed = pack_weights(make_weights(cfg, seed=5), cfg)
    off = plan_bytes(cfg, packed, tmp_path, "off.plan")       # what a process with the switch off holds: no _frag entry
    held = dict(packed)
    added = add_frag_weights(held, cfg)                      # what an Engine holds with the switch on
    assert added and all(n.endswith("_frag") for n in added)
    per_block = {n.split(".", 2)[2] for n in added if n.startswith("blocks.0.")}
    assert per_block == {"feed_forward_macaron.w_1.ln.weight_frag", "feed_forward_macaron.w_2.weight_frag", "self_attn.qkv.ln.weight_frag",
                         "self_attn.linear_out.weight_frag", "conv_module.pointwise_conv1.ln.weight_frag",
                         "conv_module.pointwise_conv2.weight_frag", "feed_forward.experts.w_1.weight_frag",
                         "feed_forward.experts.w_2.weight_frag"}
    assert not any("router" in n or "out_linear" in n or "subsampling" in n or ".conv.0." in n or ".conv.2." in n for n in added)
    for n in added:                                          # each is the packer's image of the tensor it stands beside
        src = n[:-len("_frag")]
        src = src if src in packed else src + "_sliced"
        assert torch.equal(unpack_wfrag(held[n]), packed[src])
    assert plan_bytes(cfg, held, tmp_path, "on.plan") == off
    assert add_frag_weights(held, cfg) == []                 # a second context over the same dict adds nothing
    # not taken: the field off, a 16-bit mode, a narrow model
    for c in (small_cfg(weights_frag=False), small_cfg(weight_dtype="bf16"), EncoderConfig.tiny()):
        assert add_frag_weights(dict(pack_weights(make_weights(c, seed=5), c)), c) == []


def test_config_field_is_absent_at_its_default():
    cfg = small_cfg()
    assert cfg.weights_frag is True and "weights_frag" not in cfg.to_json()
    assert EncoderConfig.from_json(cfg.to_json()) == cfg
    off = dataclasses.replace(cfg, weights_frag=False)
    assert '"weights_frag": false' in off.to_json()
    assert EncoderConfig.from_json(off.to_json()) == off
