"""Two seams of the B = 1 fp32 chain, each against the form it replaces, bit for bit.

M3_ROUTER_PREFIX: the embed half of every layer's staged router GEMM on cat([embed, LN(x)]) is run once per forward by the stage
"router_e_prefix", which leaves the accumulator registers of every (layer, tile, wave) in the workspace; the router GEMMs start
from them and walk the x half only (fp32, S <= 128 rows, De = D = 256 or 512).
M3_GLU_SIG_EPI: where the GLU is deferred to the depthwise kernel, pointwise_conv1's epilogue stores sigmoid(gate) and the
depthwise kernel's taps are one multiply each.

Neither re-orders a floating-point operation, so every comparison is np.array_equal.  The switches are read once per process:
each setting runs in a child process of its own (this file run as a script), which writes its arrays to an .npz.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3m-asr-inference_amd")

# "a": router K = 512, four waves per work-group; "b": K = 1024, eight waves and 32 experts (the headline workload's
# instantiation); "s": a pinned small shape, where neither form may be taken
MODELS = {
    "a": dict(output_dim=16, attention_dim=256, attention_heads=4, num_blocks=2, embed_heads=4, embed_dim=256, embed_linear_units=256,
              embed_blocks=1, num_experts=8, hidden_units=256),
    "b": dict(output_dim=16, attention_dim=512, attention_heads=8, num_blocks=2, embed_heads=8, embed_dim=512, embed_linear_units=256,
              embed_blocks=1, num_experts=32, hidden_units=256),
    "s": dict(output_dim=16, attention_dim=64, attention_heads=2, num_blocks=2, embed_heads=2, embed_dim=64, embed_linear_units=128,
              embed_blocks=1, num_experts=16, hidden_units=128),
}
# (model, utterance lengths, packed_rows): 100 frames = 24 rows, the second row tile with 8 live rows; 70 frames = 17 rows, the
# second tile with one live row; two unequal lengths on packed rows (rows past the live count are input-masked, row P holds the
# padded frame's constant) and on padded rows (input-masked rows inside the batch)
SHAPES = {"100": ([100], None), "70": ([70], None), "2packed": ([100, 70], None), "2padded": ([100, 70], False)}
CASES = {m + k: (m, v[0], v[1]) for m in ("a", "b") for k, v in SHAPES.items()}
CASES["s100"] = ("s", [100], None)
WIDE = [k for k in CASES if k != "s100"]
SETTINGS = {"on": {}, "prefix_off": {"M3_ROUTER_PREFIX": "0"}, "sig_off": {"M3_GLU_SIG_EPI": "0"}}
NBLOCKS = 2


def _main_block0_end(names):
    """one past the last stage that belongs to the main encoder's block 0 (fused stages are named a+b)"""
    last = max(i for i, n in enumerate(names) if any(part.startswith("blocks.0.") for part in n.split("+")))
    return last + 1


def _child(out_path):
    import torch
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    arrays, meta = {}, {}
    engines, weights = {}, {}

    def inputs(cfg, lengths):
        B, T = len(lengths), max(lengths)
        feat = torch.randn(B, T, cfg.input_dim, generator=torch.Generator().manual_seed(11)).cuda()
        return feat, torch.tensor([lengths], dtype=torch.int32).cuda()

    def live_rows(eng, lengths):
        """[S] bool: the rows that hold a real frame (packed: the first row0[B]; padded: frame < the utterance's length)"""
        lens = eng.buffer("lens", torch.int32).cpu().numpy()
        B = len(lengths)
        if B > 1 and eng.packed_rows():
            S = eng.buffer("x").numel() // eng.cfg.attention_dim
            return np.arange(S) < int(eng.buffer("row0", torch.int32)[B])
        Tp = eng.output_shape(B, max(lengths))[1]
        return (np.arange(Tp)[None, :] < lens[:, None]).reshape(-1)

    def rows(eng, name, live, dtype=torch.float32):
        a = eng.buffer(name, dtype).cpu().numpy().reshape(live.shape[0], -1).copy()
        a[~live] = 0
        return a

    def gates(eng, live, key, tag=""):
        for i in range(NBLOCKS):
            arrays["%s.gate_idx%d%s" % (key, i, tag)] = rows(eng, "blocks.%d.gate_idx" % i, live, torch.int32)
            arrays["%s.gate_value%d%s" % (key, i, tag)] = rows(eng, "blocks.%d.gate_value" % i, live)

    for key, (model, lengths, packed) in CASES.items():
        cfg = EncoderConfig(**MODELS[model])
        if model not in weights:
            weights[model] = make_weights(cfg, seed=5)
        if (model, packed) not in engines:
            engines[(model, packed)] = Engine.from_state_dict(cfg, weights[model], packed_rows=packed)
        eng = engines[(model, packed)]
        feat, flen = inputs(cfg, lengths)
        logits = eng.bind(feat, flen)
        stages = eng.stage_info()
        names = [s["name"] for s in stages]
        meta[key] = dict(stages=[[s["name"], s["kernel"], s["launches"], s["alg_bytes"], s["flops"]] for s in stages],
                         num_kernels=eng.num_kernels())
        # block 0 alone first: "dw", "x" and "xn" are rewritten by every later block
        eng.run_stages(0, _main_block0_end(names))
        torch.cuda.synchronize()
        live = live_rows(eng, lengths)
        arrays[key + ".dw"] = rows(eng, "dw", live)
        arrays[key + ".x"] = rows(eng, "x", live)
        arrays[key + ".xn0"] = rows(eng, "xn", live)
        eng.forward(use_graph=False)
        torch.cuda.synchronize()
        arrays[key + ".logits"] = logits.cpu().numpy().copy()
        arrays[key + ".embed"] = rows(eng, "embed", live)
        arrays[key + ".xn"] = rows(eng, "xn", live)
        gates(eng, live, key)
        for _ in range(3):                 # capture, then two replays
            eng.forward(use_graph=True)
        torch.cuda.synchronize()
        arrays[key + ".logits_graph"] = logits.cpu().numpy().copy()

    # forked capture (model b, one utterance): the embed encoder, with the prefix stage at its end, is the side branch
    cfg = EncoderConfig(**MODELS["b"])
    feat, flen = inputs(cfg, [100])
    forked = Engine.from_state_dict(cfg, weights["b"], fork_embed=True)
    logits = forked.bind(feat, flen)
    meta["fork"] = dict(names=forked.stage_names(), num_kernels=forked.num_kernels())
    for _ in range(3):
        logits.zero_()
        forked.forward(use_graph=True)
        forked.stream.synchronize()
    arrays["fork.logits_graph"] = logits.cpu().numpy().copy()

    # the calibration sequence (model b): run up to a layer's router, edit that router's weights in place on the engine's
    # stream, run the router stage alone, run on.  An engine of its own: the edit changes its weights.
    eng = Engine.from_state_dict(cfg, weights["b"])
    logits = eng.bind(feat, flen)
    names = eng.stage_names()
    live = np.ones(logits.shape[1], dtype=bool)
    first = 0
    with torch.cuda.stream(eng.stream):
        for li in range(NBLOCKS):
            idx = names.index("blocks.%d.moe_router" % li)
            eng.run_stages(first, idx + 1)
            w = eng.weights["blocks.%d.feed_forward.router_weights_t" % li]
            delta = 0.05 * torch.randn(w.shape, generator=torch.Generator().manual_seed(23 + li))
            w -= delta.to(w.device)
            eng.run_stages(idx, idx + 1)
            nxt = names.index("blocks.%d.moe_router" % (li + 1)) if li + 1 < NBLOCKS else len(names)
            eng.run_stages(idx + 1, nxt)                     # the rest of the layer: gate, experts, combine
            eng.stream.synchronize()
            arrays["calib.rl%d" % li] = eng.buffer("router_logits").cpu().numpy().copy()
            first = nxt
    eng.stream.synchronize()
    gates(eng, live, "calib", ".staged")
    arrays["calib.logits_staged"] = logits.cpu().numpy().copy()
    eng.forward(use_graph=False)
    torch.cuda.synchronize()
    gates(eng, live, "calib", ".whole")
    arrays["calib.logits_whole"] = logits.cpu().numpy().copy()
    np.savez(out_path, **arrays)
    print("B1_PREFIX " + json.dumps(meta))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: (meta, arrays)}: one child process per switch setting"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("M3_")}
    out = {}
    for name, env in SETTINGS.items():
        path = str(tmp_path_factory.mktemp("b1prefix") / (name + ".npz"))
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", path],
                           env=dict(base, **env), cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 0, "child %s exited with %d:\n%s" % (name, p.returncode, p.stderr[-4000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("B1_PREFIX ")][-1]
        out[name] = (json.loads(line[len("B1_PREFIX "):]), dict(np.load(path)))
    return out


BUFFERS = ["logits", "logits_graph", "embed", "xn", "xn0", "x", "dw"] + \
          ["gate_%s%d" % (k, i) for k in ("idx", "value") for i in range(NBLOCKS)]


def _same_buffers(a_on, a_off, case):
    for buf in BUFFERS:
        on, off = a_on["%s.%s" % (case, buf)], a_off["%s.%s" % (case, buf)]
        assert np.isfinite(on).all(), "%s: %s not finite" % (case, buf)
        assert np.array_equal(on, off), "%s: %s differs" % (case, buf)
    assert np.array_equal(a_on[case + ".logits"], a_on[case + ".logits_graph"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE)
def test_router_prefix_is_bit_identical(runs, case):
    (m_on, a_on), (m_off, a_off) = runs["on"], runs["prefix_off"]
    _same_buffers(a_on, a_off, case)
    on, off = m_on[case], m_off[case]
    names = [s[0] for s in on["stages"]]
    # exactly one more stage and one more launch, behind the last embed stage and in front of the first router
    assert names.count("router_e_prefix") == 1 and "router_e_prefix" not in [s[0] for s in off["stages"]]
    at = names.index("router_e_prefix")
    assert on["stages"][at][1] == "router_embed_prefix_kernel" and on["stages"][at][2] == 1
    assert on["num_kernels"] - off["num_kernels"] == 1
    assert max(i for i, n in enumerate(names) if any(p.startswith("embed.") for p in n.split("+"))) < at
    assert at < min(i for i, n in enumerate(names) if n.endswith(".moe_router"))
    rest = on["stages"][:at] + on["stages"][at + 1:]
    assert [s[:3] for s in rest] == [s[:3] for s in off["stages"]]
    # the routers keep name and label; the embed half's FLOPs moved to the prefix stage, nothing else changed
    r_on = [s for s in rest if s[0].endswith(".moe_router")]
    r_off = [s for s in off["stages"] if s[0].endswith(".moe_router")]
    assert len(r_on) == NBLOCKS and all(s[1] == "gemm_f32_kernel" for s in r_on + r_off)
    assert sum(s[4] for s in r_on) + on["stages"][at][4] == sum(s[4] for s in r_off)
    assert all(a[4] == b[4] / 2 for a, b in zip(r_on, r_off))              # De = D: half the K
    assert [s for s in rest if not s[0].endswith(".moe_router")] == [s for s in off["stages"] if not s[0].endswith(".moe_router")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE)
def test_glu_sigmoid_in_pw1_epilogue_is_bit_identical(runs, case):
    (m_on, a_on), (m_off, a_off) = runs["on"], runs["sig_off"]
    _same_buffers(a_on, a_off, case)
    assert m_on[case] == m_off[case]                 # the stage lists are entry for entry equal
    assert any("conv.pw1_glu" in s[0] and s[1] in ("gemm_f32_kernel", "gemm_f32_dual_kernel") for s in m_on[case]["stages"])


@pytest.mark.gpu
def test_small_shapes_keep_their_stage_list(runs):
    """D = 64: the same stage list, entry for entry, and the same logits under every setting"""
    ref_meta, ref = runs["on"][0]["s100"], runs["on"][1]
    assert "router_e_prefix" not in [s[0] for s in ref_meta["stages"]]
    for name in ("prefix_off", "sig_off"):
        assert runs[name][0]["s100"] == ref_meta, name
        for buf in ("logits", "logits_graph"):
            assert np.array_equal(runs[name][1]["s100." + buf], ref["s100." + buf]), (name, buf)


@pytest.mark.gpu
def test_forked_capture_joins_behind_the_prefix_stage(runs):
    """fork_embed: the prefix stage ends the embed branch; the forked graph's logits after three replays are the chain's"""
    for name, (meta, a) in runs.items():
        assert np.array_equal(a["fork.logits_graph"], a["b100.logits"]), name
        assert np.array_equal(a["fork.logits_graph"], runs["prefix_off"][1]["b100.logits"]), name
    names = runs["on"][0]["fork"]["names"]
    at = names.index("router_e_prefix")
    assert names[at - 1].startswith("embed.") and names[at + 1].startswith("subsample.")
    assert "router_e_prefix" not in runs["prefix_off"][0]["fork"]["names"]
    assert runs["on"][0]["fork"]["num_kernels"] - runs["prefix_off"][0]["fork"]["num_kernels"] == 1


@pytest.mark.gpu
def test_router_rerun_after_a_weight_edit_sees_no_stale_prefix(runs):
    """The calibration's sequence: stages up to a layer's router, the router's weights edited in place, the router stage alone,
    the rest -- a prefix formed from the old weights must not meet the new x columns."""
    a_on, a_off = runs["on"][1], runs["prefix_off"][1]
    keys = ["calib.rl%d" % i for i in range(NBLOCKS)] + ["calib.logits_staged", "calib.logits_whole"] + \
           ["calib.gate_%s%d.%s" % (k, i, t) for k in ("idx", "value") for i in range(NBLOCKS) for t in ("staged", "whole")]
    for k in keys:
        assert np.isfinite(a_on[k]).all(), k
        assert np.array_equal(a_on[k], a_off[k]), k + " differs"
    assert np.array_equal(a_on["calib.logits_staged"], a_on["calib.logits_whole"])
    # (the edit does change the routing input: the comparison above is not between two untouched routers)
    assert not np.array_equal(a_on["calib.gate_value0.staged"], a_on["b100.gate_value0"])


if __name__ == "__main__":
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: test_b1_router_prefix_gpu.py --child OUT.npz")
