"""Horizontal fusion of the fp32 engine (M3_HFUSE: stages of the embed encoder paired with stages of the main encoder's prefix,
one launch per pair) against M3_HFUSE=0, bit for bit, on models whose two encoders DIFFER in shape.

tests/test_b1_chain_gpu.py compares engines whose halves have one shape; tests/test_stage_list_gpu.py sets M3_HFUSE=0 but compares
stage lists only.  Here the embed encoder has other head widths (dk 128 against 64, and the mirror: the <128, 64> and <64, 128>
instantiations of relpos_attention_dual_kernel) and another feed-forward width (384 against 256) than the main encoder, so the
greedy partner search pairs GEMMs of unequal M x N x K, and the inputs give 24 rows (100 frames), 17 rows (70 frames: a second
row tile with one live row) and two padded utterances (48 rows, input-masked rows inside the batch).

Pairing re-orders no arithmetic, so every comparison is np.array_equal.  The switch is read once per process: each setting runs
in a child process of its own (this file run as a script), which writes its arrays to an .npz the test compares.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3m-asr-inference_amd")

_COMMON = dict(output_dim=16, attention_dim=256, num_blocks=2, embed_dim=256, embed_linear_units=384, embed_blocks=2, num_experts=8,
               hidden_units=256)
MODELS = {
    "m1": dict(_COMMON, attention_heads=4, embed_heads=2),      # main dk 64, embed dk 128
    "m2": dict(_COMMON, attention_heads=2, embed_heads=4),      # the mirror
}
# (utterance lengths, packed_rows)
INPUTS = {"b1_100": ([100], None), "b1_70": ([70], None), "b2_padded": ([100, 70], False)}
CASES = [(m, i) for m in MODELS for i in INPUTS]
SETTINGS = {"on": {}, "off": {"M3_HFUSE": "0"}}
BUFFERS = ("x", "embed", "lens", "logits", "logits_graph")
DUAL_KERNELS = ("gemm_f32_dual_kernel", "dwconv_ln_silu_dual_kernel", "relpos_attention_dual_kernel")


def _child(out_path):
    import torch
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    arrays, meta, engines = {}, {}, {}
    for model, inp in CASES:
        lengths, packed = INPUTS[inp]
        key = model + "." + inp
        cfg = EncoderConfig(**MODELS[model])
        if (model, packed) not in engines:
            engines[(model, packed)] = Engine.from_state_dict(cfg, make_weights(cfg, seed=5), packed_rows=packed)
        eng = engines[(model, packed)]
        B, T = len(lengths), max(lengths)
        g = torch.Generator().manual_seed(11)
        feat = torch.randn(B, T, cfg.input_dim, generator=g).cuda()
        flen = torch.tensor([lengths], dtype=torch.int32).cuda()
        logits = eng.bind(feat, flen)
        meta[key] = dict(stages=[[s["name"], s["kernel"], s["launches"], s["alg_bytes"], s["flops"]] for s in eng.stage_info()],
                         num_kernels=eng.num_kernels())
        eng.forward(use_graph=False)
        torch.cuda.synchronize()
        arrays[key + ".logits"] = logits.cpu().numpy().copy()
        arrays[key + ".x"] = eng.buffer("x").cpu().numpy().copy()
        arrays[key + ".embed"] = eng.buffer("embed").cpu().numpy().copy()
        arrays[key + ".lens"] = eng.buffer("lens", torch.int32).cpu().numpy().copy()
        eng.forward(use_graph=True)        # the captured graph replays the same launches
        torch.cuda.synchronize()
        arrays[key + ".logits_graph"] = logits.cpu().numpy().copy()
    np.savez(out_path, **arrays)
    print("HFUSE " + json.dumps(meta))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: (meta, arrays)}: one child process per switch setting"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("M3_")}
    out = {}
    for name, env in SETTINGS.items():
        path = str(tmp_path_factory.mktemp("hfuse") / (name + ".npz"))
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", path],
                           env=dict(base, **env), cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 0, "child %s exited with %d:\n%s" % (name, p.returncode, p.stderr[-4000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("HFUSE ")][-1]
        out[name] = (json.loads(line[len("HFUSE "):]), dict(np.load(path)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("model,inp", CASES)
def test_hfuse_is_bit_identical(runs, model, inp):
    (m_on, a_on), (m_off, a_off) = runs["on"], runs["off"]
    key = model + "." + inp
    for buf in BUFFERS:
        on, off = a_on["%s.%s" % (key, buf)], a_off["%s.%s" % (key, buf)]
        assert np.isfinite(on.astype(np.float64)).all(), "%s: %s is not finite" % (key, buf)
        assert on.shape == off.shape and np.array_equal(on, off), "%s: %s differs between M3_HFUSE on and off" % (key, buf)
    assert np.array_equal(a_on[key + ".logits"], a_on[key + ".logits_graph"])
    assert np.array_equal(a_off[key + ".logits"], a_off[key + ".logits_graph"])


@pytest.mark.gpu
@pytest.mark.parametrize("model,inp", CASES)
def test_hfuse_stage_lists(runs, model, inp):
    key = model + "." + inp
    on, off = runs["on"][0][key], runs["off"][0][key]
    fused = [s for s in on["stages"] if "+" in s[0]]
    assert not any("+" in s[0] for s in off["stages"])
    assert all(s[2] == 1 for s in fused)                        # every stage named a+b is one launch in place of two
    for kernel in DUAL_KERNELS:
        assert any(s[1] == kernel for s in fused), "%s: no a+b stage runs %s" % (key, kernel)
    # both halves of every pair are stages of the unfused list, the embed encoder's first
    by_name_off = {s[0]: s for s in off["stages"]}
    for s in fused:
        a, b = s[0].split("+")
        assert a.startswith("embed.") and not b.startswith("embed.") and {a, b} <= set(by_name_off), s[0]
        # ... and a pair's algorithmic bytes and FLOPs are its halves' (exact: the same doubles summed in the same order)
        assert s[3] == by_name_off[a][3] + by_name_off[b][3] and s[4] == by_name_off[a][4] + by_name_off[b][4], s[0]
    assert off["num_kernels"] - on["num_kernels"] == len(fused)
    assert sum(s[2] for s in off["stages"]) - sum(s[2] for s in on["stages"]) == len(fused)


@pytest.mark.gpu
def test_both_mixed_attention_instantiations_are_reached(runs):
    """model m1 pairs an embed attention of dk 128 with a main attention of dk 64, m2 the mirror: the <128, 64> and <64, 128> forms"""
    from m3asr.config import EncoderConfig
    widths = {m: (EncoderConfig(**MODELS[m]).embed_dim // MODELS[m]["embed_heads"], MODELS[m]["attention_dim"] // MODELS[m]["attention_heads"])
              for m in MODELS}
    assert widths == {"m1": (128, 64), "m2": (64, 128)}
    for m in MODELS:
        stages = runs["on"][0][m + ".b1_100"]["stages"]
        assert [s[0] for s in stages if s[1] == "relpos_attention_dual_kernel"] == ["embed.blocks.0.att.core+blocks.0.att.core"], m


if __name__ == "__main__":
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: test_hfuse_gpu.py --child OUT.npz")
