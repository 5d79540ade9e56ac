"""Fragment-ordered fp32 weights on the device (include/m3asr.h "fragment order"): every kernel that reads them
against the same kernel on the row-major / slice-major tensors.  No floating-point operation moves -- each lane receives the
16 bytes it received before -- so every comparison is bit for bit (guarded.same_bits / np.array_equal), never a tolerance.

  m3_linear_wfrag / m3_linear_pair_wfrag   against m3_linear / the single launches, on guarded row-strided operands
  m3_moe_route_expert_ffn (w2_sliced = 2)  against w2_sliced = 1: the result rows and the partial-result slabs
  m3_moe_expert_ffn_wfrag                  against m3_moe_expert_ffn (the staged slab form)
  the engine                               M3_W_FRAG = 1 against 0 in child processes

GEMM shapes, from skinny_grid / gemm_group_steps (csrc/gemm_plan.hip, kernels.h): K = 16 is one K-step (waves 1..3 of the four
re-load it through the clamp), K = 80 five ragged steps, K = 512 / 1024 the full single group at 4 / 8 waves, K = 2048 sixteen
waves with two groups (double-buffered); M = 200 plans 32-row tiles, M = 600 at K = 80 64-row tiles; N = 1024 takes the XCD
swizzle (64 column tiles), N = 16 / 48 do not.  sig_col0 has no field in m3_linear_desc: the engine cases run it (pw1 at D >= 256).

Seeded faults.  kq and col swapped in pack_wfrag: run, fails tests/test_wfrag_host.py (the index formula) and would fail every
case here.  The other two make the kernel read outside the weight tensor, so they were reasoned, not run on a device: without
the clamp on the last K-step the waves past K / 16 (K = 16: three of four; K = 80: steps 5..7) load the next column tile's KB or
the bytes behind the tensor instead of re-loading a step whose result is unused -- harmless to the values, a fault at the last
tile; the GLU half addressed by Nout instead of Nout / 16 tiles reads gate weights 16 times too far in: every GLU case's values."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3m-asr-inference_amd")


def rnd(*shape, seed=0, scale=1.0):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ================================================================================================ skinny GEMM
# (M, N, K, epilogue)
GEMM_CASES = [
    (1, 16, 16, "plain"), (17, 48, 80, "plain"), (50, 1024, 512, "plain"), (50, 1024, 1024, "plain"), (50, 48, 2048, "plain"),
    (50, 1024, 2048, "resid"), (17, 16, 512, "silu"), (1, 1024, 80, "resid"), (50, 48, 1024, "ln_mask"), (50, 1024, 512, "ln_mask"),
    (17, 96, 80, "glu"), (50, 2048, 512, "glu_ln_mask"), (50, 32, 16, "glu"), (50, 2048, 1024, "glu"), (17, 1024, 16, "silu"),
    (200, 1024, 512, "resid"), (200, 2048, 512, "glu"), (600, 1024, 80, "plain"), (600, 2048, 80, "glu"), (200, 1024, 2048, "plain"),
]


def gemm_problem(M, N, K, epi, seed, frag):
    """-> (keyword arguments of ops.linear, the guarded output)"""
    import torch
    import guarded as G
    from m3asr import _lib
    from m3asr.plan import fold_layernorm, pack_wfrag
    glu = epi.startswith("glu")
    n_out = N // 2 if glu else N
    a = G.strided_in(rnd(M, K, seed=seed))
    w, b = rnd(N, K, seed=seed + 1, scale=K ** -0.5), rnd(N, seed=seed + 2)
    kw = dict(act=_lib.ACT_GLU if glu else (_lib.ACT_SILU if epi == "silu" else _lib.ACT_NONE))
    if "ln" in epi:
        f = fold_layernorm(w, b, 1.0 + 0.1 * rnd(K, seed=seed + 3), 0.1 * rnd(K, seed=seed + 4))
        w, b = f["ln.weight"], f["ln.bias"]
        kw["ln_folded"] = (f["ln.wsum"].cuda(), f["ln.wbeta"].cuda(), 1e-5)
    if "mask" in epi:      # rows of 1..M frames: the last third of them padding
        kw.update(lens=torch.tensor([max(1, M - M // 3)], dtype=torch.int32).cuda(), rows_per_batch=M, mask_in=True)
    if epi == "resid":
        kw.update(resid=G.strided_in(rnd(M, n_out, seed=seed + 5)).view, alpha=0.5)
    out = G.strided_out(M, n_out)
    wd = w.cuda().contiguous()
    kw.update(a=a.view, w=pack_wfrag(wd) if frag else wd, bias=b.cuda(), out=out.view)
    return kw, out


def launch_linear(kw):
    from m3asr import ops
    kw = dict(kw)
    return ops.linear(kw.pop("a"), kw.pop("w"), **kw)


def written_and_guarded(out, what):
    out.check(what)
    assert not bool(out.untouched().any()), "%s: %d element(s) never written" % (what, int(out.untouched().sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,epi", GEMM_CASES, ids=["%dx%dx%d-%s" % c for c in GEMM_CASES])
def test_linear_wfrag_equals_linear(M, N, K, epi):
    import torch
    import guarded as G
    from m3asr import ops
    outs = []
    for frag in (False, True):
        kw, out = gemm_problem(M, N, K, epi, seed=3, frag=frag)
        k2 = dict(kw)
        assert ops.linear_kernel(k2.pop("a"), k2.pop("w"), **k2) == "gemm_f32_kernel"
        launch_linear(kw)
        torch.cuda.synchronize()
        written_and_guarded(out, "frag=%s" % frag)
        outs.append(out)
    assert bool(torch.isfinite(outs[0].view).all())
    assert G.same_bits(outs[0].view, outs[1].view), "max abs diff %g" % float((outs[0].view - outs[1].view).abs().max())


# the instantiations gemm_f32_dual_kernel has: 16-row tiles, 4 / 8 waves, plain / GLU, with / without the folded LayerNorm;
# two unequal problems each
PAIR_CASES = [((50, 1024, 512, "plain"), (17, 48, 80, "silu")), ((50, 512, 1024, "resid"), (1, 1024, 1024, "plain")),
              ((50, 2048, 512, "glu_ln_mask"), (17, 96, 512, "glu_ln_mask")), ((50, 1024, 512, "ln_mask"), (24, 48, 512, "ln_mask")),
              ((50, 96, 80, "glu"), (17, 2048, 16, "glu"))]


@pytest.mark.gpu
@pytest.mark.parametrize("pa,pb", PAIR_CASES, ids=["%dx%dx%d-%s+%dx%dx%d-%s" % (a + b) for a, b in PAIR_CASES])
def test_linear_pair_wfrag_equals_singles(pa, pb):
    import torch
    import guarded as G
    from m3asr import ops
    ref = []
    for i, p in enumerate((pa, pb)):
        kw, out = gemm_problem(*p, seed=7 + 10 * i, frag=False)
        launch_linear(kw)
        ref.append(out)
    for order in ((0, 1), (1, 0)):
        probs = [gemm_problem(*(pa, pb)[i], seed=7 + 10 * i, frag=True) for i in order]
        ops.linear_pair(probs[0][0], probs[1][0])
        torch.cuda.synchronize()
        for i, (kw, out) in zip(order, probs):
            written_and_guarded(out, "pair %s problem %d" % (order, i))
            assert G.same_bits(out.view, ref[i].view), "pair %s problem %d differs from the single row-major launch" % (order, i)
    # the two problems must agree on the layout: the launcher refuses a mixed pair (the wrapper would not build one)
    ka, _ = gemm_problem(*pa, seed=7, frag=True)
    kb, _ = gemm_problem(*pb, seed=17, frag=False)
    with pytest.raises(AssertionError):
        ops.linear_pair(ka, kb)


# ================================================================================================ expert FFN
E, D = 8, 256


def expert_weights(F, D_=D, seed=21):
    from m3asr.plan import pack_wfrag, slice_major_w2
    w1, b1 = rnd(E, F, D_, seed=seed, scale=D_ ** -0.5).cuda(), rnd(E, F, seed=seed + 1).cuda()
    w2, b2 = rnd(E, D_, F, seed=seed + 2, scale=F ** -0.5).cuda(), rnd(E, D_, seed=seed + 3).cuda()
    w2s = slice_major_w2(w2)
    return dict(w1=w1, b1=b1, w2=w2, w2s=w2s, b2=b2, w1f=pack_wfrag(w1), w2f=pack_wfrag(w2s))


def routing_logits(S, seed, empty=(2, 5)):
    lg = rnd(S, E, seed=seed)
    lg[:, list(empty)] = -30.0          # two experts receive no row
    return lg.cuda()


# S = 3 / 50 / 64: every wave routes for itself; 65 / 100: the per-work-group prologue; D = 272: 17 output tiles (no multiple of 8)
ROUTE_CASES = [(S, F, D) for F in (64, 128) for S in (3, 50, 64, 65, 100)] + [(50, 64, 272)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,F,D_", ROUTE_CASES, ids=["S%d-F%d-D%d" % c for c in ROUTE_CASES])
def test_self_routing_expert_wfrag(S, F, D_):
    import torch
    import guarded as G
    from m3asr import ops
    w = expert_weights(F, D_)
    logits = routing_logits(S, seed=31 + S)
    g, bta = (1.0 + 0.1 * rnd(D_, seed=5)).cuda(), (0.1 * rnd(D_, seed=6)).cuda()
    res = []
    for frag in (False, True):
        x = G.strided_in(rnd(S, D_, seed=33))
        ws = torch.zeros(ops.moe_route_expert_workspace_size(S, E, D_, F), dtype=torch.uint8, device="cuda")
        y = torch.empty(S, D_, device="cuda")
        y, taps = ops.moe_route_expert_ffn(x.view, logits, w["w1f"] if frag else w["w1"], w["b1"], w["w2f"] if frag else w["w2s"], w["b2"],
                                           w2_sliced=True, resid=rnd(S, D_, seed=34).cuda(), alpha=0.5, ln=(g, bta, 1e-5), workspace=ws, out=y)
        torch.cuda.synchronize()
        res.append((y, ws, taps))
    (y0, ws0, t0), (y1, ws1, t1) = res
    assert bool(torch.isfinite(y0).all())
    hist = t0[3].cpu().numpy()
    assert hist[3] == hist[2] and hist[6] == hist[5], "experts 2 and 5 were meant to stay empty: %s" % hist
    assert torch.equal(ws0, ws1), "the partial-result slabs differ"
    assert G.same_bits(y0, y1), "the combined rows differ"
    for a, b in zip(t0, t1):
        assert torch.equal(a, b)


SLAB_CASES = [(3, 64), (50, 128), (65, 64), (100, 128), (600, 64)]      # 16-, 32- and (600 rows) 64-row tiles of the staged form


@pytest.mark.gpu
@pytest.mark.parametrize("S,F", SLAB_CASES, ids=["S%d-F%d" % c for c in SLAB_CASES])
def test_staged_expert_wfrag(S, F):
    import torch
    import guarded as G
    from m3asr import ops
    w = expert_weights(F)
    gate = routing_logits(S, seed=41 + S).argmax(1).to(torch.int32)
    gate[S // 2] = -1                      # a dropped row
    x = rnd(S, D, seed=43).cuda()
    res = []
    for frag in (False, True):
        ws = torch.zeros(ops.moe_expert_workspace_size(S, E, D, F), dtype=torch.uint8, device="cuda")
        y = ops.moe_expert_ffn(x, gate, w["w1f"] if frag else w["w1"], w["b1"], w["w2f"] if frag else w["w2"], w["b2"], workspace=ws)
        torch.cuda.synchronize()
        res.append((y, ws))
    assert bool(torch.isfinite(res[0][0]).all())
    assert torch.equal(res[0][1], res[1][1]), "the workspace (index + partial-result slabs) differs"
    assert G.same_bits(res[0][0], res[1][0])


@pytest.mark.gpu
def test_staged_expert_wfrag_refuses_the_tiled_form():
    import torch
    from m3asr import ops
    from m3asr._lib import M3Error
    S, F = 1024, 128                       # M3_EXPERT_TILED_MIN_ROWS rows and room for H: two grouped GEMMs, which read the slice-major tensors
    w = expert_weights(F)
    gate = torch.zeros(S, dtype=torch.int32, device="cuda")
    with pytest.raises(M3Error, match="fragment-ordered weights exist for the fp32 slab form only"):
        ops.moe_expert_ffn(rnd(S, D, seed=1).cuda(), gate, w["w1f"], w["b1"], w["w2f"], w["b2"])


# ================================================================================================ engine
MODELS = {
    "a": dict(output_dim=16, attention_dim=256, attention_heads=4, num_blocks=2, embed_heads=4, embed_dim=256, embed_linear_units=256,
              embed_blocks=1, num_experts=8, hidden_units=256),
    "b": dict(output_dim=16, attention_dim=512, attention_heads=8, num_blocks=2, embed_heads=8, embed_dim=512, embed_linear_units=256,
              embed_blocks=1, num_experts=8, hidden_units=256),
}
# 100 frames = 24 rows; a ragged pair padded and packed; 1610 frames = 401 rows: the block GEMMs plan tiled (>= 384 rows, >= 160 tiles)
ENGINE_CASES = {m + k: (m, l, p) for m in ("a", "b") for k, (l, p) in
                {"100": ([100], None), "2packed": ([100, 70], None), "2padded": ([100, 70], False)}.items()}
ENGINE_CASES["b1610"] = ("b", [1610], None)
NBLOCKS = 2


def _child(out_path):
    import torch
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    arrays, meta, engines, weights = {}, {}, {}, {}
    for key, (model, lengths, packed) in ENGINE_CASES.items():
        cfg = EncoderConfig(**MODELS[model])
        if model not in weights:
            weights[model] = make_weights(cfg, seed=5)
        if (model, packed) not in engines:
            engines[(model, packed)] = Engine.from_state_dict(cfg, weights[model], packed_rows=packed)
        eng = engines[(model, packed)]
        B, T = len(lengths), max(lengths)
        feat = torch.randn(B, T, cfg.input_dim, generator=torch.Generator().manual_seed(11)).cuda()
        logits = eng.bind(feat, torch.tensor([lengths], dtype=torch.int32).cuda())
        stages = eng.stage_info()
        names = [s["name"] for s in stages]
        meta[key] = dict(stages=[[s["name"], s["kernel"], s["launches"], s["alg_bytes"], s["flops"]] for s in stages],
                         num_kernels=eng.num_kernels())
        end0 = max(i for i, n in enumerate(names) if any(part.startswith("blocks.0.") for part in n.split("+"))) + 1
        eng.run_stages(0, end0)
        torch.cuda.synchronize()
        arrays[key + ".x0"] = eng.buffer("x").cpu().numpy().copy()
        eng.forward(use_graph=False)
        torch.cuda.synchronize()
        arrays[key + ".logits"] = logits.cpu().numpy().copy()
        for i in range(NBLOCKS):
            arrays["%s.gate_idx%d" % (key, i)] = eng.buffer("blocks.%d.gate_idx" % i, torch.int32).cpu().numpy().copy()
        for _ in range(3):                 # capture, then two replays
            eng.forward(use_graph=True)
        torch.cuda.synchronize()
        arrays[key + ".logits_graph"] = logits.cpu().numpy().copy()
    eng = engines[("b", None)]
    clone = eng.clone_context()
    frag = sorted(n for n in eng.weights if n.endswith("_frag"))
    meta["frag_names"] = frag
    meta["clone_shares"] = all(clone.weights[n].data_ptr() == eng.weights[n].data_ptr() for n in eng.weights) and \
        sorted(clone.weights) == sorted(eng.weights)
    np.savez(out_path, **arrays)
    print("WFRAG " + json.dumps(meta))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"on" / "off": (meta, arrays)}: one child process per setting of M3_W_FRAG"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("M3_")}
    out = {}
    for name, env in {"on": {}, "off": {"M3_W_FRAG": "0"}}.items():
        path = str(tmp_path_factory.mktemp("wfrag") / (name + ".npz"))
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", path],
                           env=dict(base, **env), cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 0, "child %s exited with %d:\n%s" % (name, p.returncode, p.stderr[-4000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("WFRAG ")][-1]
        out[name] = (json.loads(line[len("WFRAG "):]), dict(np.load(path)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_switch_on_equals_off(runs, case):
    (m_on, a_on), (m_off, a_off) = runs["on"], runs["off"]
    for buf in ["logits", "logits_graph", "x0"] + ["gate_idx%d" % i for i in range(NBLOCKS)]:
        on, off = a_on["%s.%s" % (case, buf)], a_off["%s.%s" % (case, buf)]
        assert np.isfinite(on).all(), "%s: %s not finite" % (case, buf)
        assert np.array_equal(on, off), "%s: %s differs" % (case, buf)
    assert np.array_equal(a_on[case + ".logits"], a_on[case + ".logits_graph"])
    # names, family labels, launch counts, alg_bytes and FLOPs of every stage: unchanged
    assert m_on[case] == m_off[case]


@pytest.mark.gpu
def test_engine_holds_and_shares_the_fragment_tensors(runs):
    m_on, m_off = runs["on"][0], runs["off"][0]
    assert m_off["frag_names"] == []
    per_block = {n.split(".", 2)[2] for n in m_on["frag_names"] if n.startswith("blocks.1.")}
    assert per_block == {"feed_forward_macaron.w_1.ln.weight_frag", "feed_forward_macaron.w_2.weight_frag", "self_attn.qkv.ln.weight_frag",
                         "self_attn.linear_out.weight_frag", "conv_module.pointwise_conv1.ln.weight_frag",
                         "conv_module.pointwise_conv2.weight_frag", "feed_forward.experts.w_1.weight_frag",
                         "feed_forward.experts.w_2.weight_frag"}
    assert m_on["clone_shares"] and m_off["clone_shares"]


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    sys.path.insert(0, PKG)
    _child(sys.argv[2])
