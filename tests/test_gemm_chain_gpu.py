"""The skinny fp32 GEMM's work-group chain: the row mask asked for up front and resolved in the epilogue, the
16-row tile's epilogue spread over four waves, the router's normalised rows stored behind its MFMAs, the tile order by a
host-made multiplier.  None of them re-orders a floating-point operation, so wherever two launches of the kernel are compared
the comparison is np.array_equal; against fp64 the bounds are those of tests/test_kernels_gpu.py.

Shapes: 17 and 50 rows (a ragged last 16-row tile; 50 rows are four tiles), K = 512 / 1024 / 2048 (4 / 8 / 16 waves per
work-group; GLU and the folded LayerNorm have no 16-wave form and run K = 2048 on 8 waves with two load groups), N = 32, 48 (no
multiple of 32) and 26 (no multiple of 16: the `ep_n < Nout` guard).  Fragment-ordered weights need N % 16 == 0.

Not reachable from ops.linear and therefore covered through the engine below: `sig_col0` (pointwise_conv1 of the 256- and
512-wide configs stores sigmoid(gate) for the columns from D on, a 16-column boundary) and `acc_init` (the routers of the same
configs start from the embed prefix).  tests/test_b1_router_prefix_gpu.py compares both with their switches off, in child
processes; here the router runs with and without the prefix in two child processes as well, up to block 0's router only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

KS = [512, 1024, 2048]
NS = [32, 48, 26]
MS = [17, 50]
# (M, rows_per_batch, lengths): one utterance of 50; two utterances of 25 rows whose lengths end inside a quad of rows / whose
# boundary (row 25) cuts the quad 24 .. 27; rows_per_batch >= M (one run: no division in the kernel) with every, some and no
# live row; 17 rows as one run and as 9 + 8
LENGTHS = [(50, 50, [50]), (50, 25, [25, 9]), (50, 25, [23, 25]), (50, 25, [1, 25]), (50, 64, [50]), (50, 64, [37]), (50, 64, [0]),
           (17, 17, [9]), (17, 9, [9, 3])]


def _t():
    import torch
    import torch.nn.functional as F
    from m3asr import ops, _lib
    return torch, F, ops, _lib


def rnd(*shape, seed=0, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.cuda().contiguous()


def close(got, want, rtol, atol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    print("%s max abs err %.3e (max |ref| %.3e)" % (what, float(err.max()), float(want.abs().max())))
    assert bool((err <= bound).all()), "%s max abs err %.3e (max |ref| %.3e), worst excess %.3e" % (
        what, float(err.max()), float(want.abs().max()), float((err - bound).max()))


def same(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _pad_rows(M, rpb, lens):
    m = np.arange(M)
    return np.asarray(lens)[m // rpb] <= (m % rpb)


def _skinny(ops, *a, **kw):
    assert ops.linear_kernel(*a, **kw) == "gemm_f32_kernel", "the shape left the skinny fp32 kernel"


# ================================================================================================ the row mask
@pytest.mark.parametrize("K", KS)
def test_mask_out_is_the_unmasked_launch_on_live_rows(K):
    torch, F, ops, _lib = _t()
    for N in NS:
        for M, rpb, lens in LENGTHS:
            a, w, b, res = dev(rnd(M, K, seed=1)), dev(rnd(N, K, seed=2, scale=K ** -0.5)), dev(rnd(N, seed=3)), dev(rnd(M, N, seed=4))
            ln = dev(torch.tensor(lens, dtype=torch.int32))
            pad = _pad_rows(M, rpb, lens)
            for resid in (None, res):
                kw = dict(act=_lib.ACT_SILU, alpha=0.5, resid=resid)
                _skinny(ops, a, w, b, lens=ln, rows_per_batch=rpb, mask_out=True, **kw)
                plain = ops.linear(a, w, b, **kw).cpu().numpy()
                got = ops.linear(a, w, b, lens=ln, rows_per_batch=rpb, mask_out=True, **kw).cpu().numpy()
                what = "K=%d N=%d M=%d rpb=%d lens=%s resid=%s" % (K, N, M, rpb, lens, resid is not None)
                assert np.array_equal(got[~pad], plain[~pad]), what + ": live rows"
                fill = res.cpu().numpy()[pad] if resid is not None else np.zeros((int(pad.sum()), N), np.float32)
                assert np.array_equal(got[pad], fill), what + ": padded rows"


@pytest.mark.parametrize("K", KS)
def test_mask_in_plain(K):
    """live rows: the unmasked launch; padded rows: a zero accumulator, i.e. the bias through the activation"""
    torch, F, ops, _lib = _t()
    for N in NS:
        for M, rpb, lens in LENGTHS:
            a, w, b = dev(rnd(M, K, seed=1)), dev(rnd(N, K, seed=2, scale=K ** -0.5)), dev(rnd(N, seed=3))
            ln = dev(torch.tensor(lens, dtype=torch.int32))
            pad = _pad_rows(M, rpb, lens)
            for act in (_lib.ACT_NONE, _lib.ACT_RELU):
                plain = ops.linear(a, w, b, act=act).cpu().numpy()
                got = ops.linear(a, w, b, act=act, lens=ln, rows_per_batch=rpb, mask_in=True).cpu().numpy()
                what = "K=%d N=%d M=%d rpb=%d lens=%s act=%d" % (K, N, M, rpb, lens, act)
                assert np.array_equal(got[~pad], plain[~pad]), what + ": live rows"
                bias = b.cpu().numpy()
                want = np.maximum(bias, 0) if act == _lib.ACT_RELU else bias
                assert np.array_equal(got[pad], np.broadcast_to(want, (int(pad.sum()), N))), what + ": padded rows"


@pytest.mark.parametrize("K", [512, 1024])
def test_mask_in_folded_layernorm(K):
    """(the folded LayerNorm is built for K < 2048.)  padded rows: masked_fill(0) behind the LayerNorm, -wbeta + bias"""
    torch, F, ops, _lib = _t()
    from m3asr.plan import fold_layernorm
    for N in NS:
        w, b = rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
        f = fold_layernorm(w, b, rnd(K, seed=5) * 0.2 + 1.0, rnd(K, seed=6, scale=0.1))
        wf, bf, wsum, wbeta = dev(f["ln.weight"]), dev(f["ln.bias"]), dev(f["ln.wsum"]), dev(f["ln.wbeta"])
        for M, rpb, lens in LENGTHS:
            a = dev(rnd(M, K, seed=1) * 1.7 + 0.4)
            ln = dev(torch.tensor(lens, dtype=torch.int32))
            pad = _pad_rows(M, rpb, lens)
            _skinny(ops, a, wf, bf, ln_folded=(wsum, wbeta, 1e-12), lens=ln, rows_per_batch=rpb, mask_in=True)
            plain = ops.linear(a, wf, bf, ln_folded=(wsum, None, 1e-12)).cpu().numpy()
            got = ops.linear(a, wf, bf, ln_folded=(wsum, wbeta, 1e-12), lens=ln, rows_per_batch=rpb, mask_in=True).cpu().numpy()
            what = "K=%d N=%d M=%d rpb=%d lens=%s" % (K, N, M, rpb, lens)
            assert np.array_equal(got[~pad], plain[~pad]), what + ": live rows"
            want = ((-wbeta) + bf).cpu().numpy()
            assert np.array_equal(got[pad], np.broadcast_to(want, (int(pad.sum()), N))), what + ": padded rows"


# ================================================================================================ the epilogue
def _act_ref(F, lin, act, _lib, n_out):
    if act == _lib.ACT_GLU:
        return F.glu(lin, -1)
    return {_lib.ACT_NONE: lin, _lib.ACT_RELU: F.relu(lin), _lib.ACT_SILU: F.silu(lin)}[act]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("act_name", ["none", "relu", "silu", "glu"])
def test_epilogue_every_activation(K, act_name):
    """alpha = 0.5 and an in-place residual (Y aliases resid, as the engine's residual stream does) on guarded, row-strided
    operands: fp64 parity, fragment-ordered W == row-major W bit for bit, and not a byte outside the M x N output written
    (the spread epilogue has four waves storing where one did)."""
    import guarded as G
    torch, F, ops, _lib = _t()
    from m3asr.plan import pack_wfrag
    act = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "silu": _lib.ACT_SILU, "glu": _lib.ACT_GLU}[act_name]
    glu = act == _lib.ACT_GLU
    for M in MS:
        for n_out in NS:
            N = 2 * n_out if glu else n_out
            a, w, b, res = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, n_out, seed=4)
            want = res.double() + 0.5 * _act_ref(F, F.linear(a.double(), w.double(), b.double()), act, _lib, n_out)
            ga = G.strided_in(a)
            what = "K=%d act=%s M=%d n_out=%d" % (K, act_name, M, n_out)
            _skinny(ops, ga.view, dev(w), dev(b), act=act, alpha=0.5)
            outs = []
            for frag in ([False, True] if n_out % 16 == 0 else [False]):
                gy = G.strided_out(M, n_out)
                gy.view.copy_(res.cuda())
                wd = pack_wfrag(dev(w)) if frag else dev(w)
                y = ops.linear(ga.view, wd, dev(b), act=act, alpha=0.5, resid=gy.view, out=gy.view)
                torch.cuda.synchronize()
                gy.check(what + " frag=%s" % frag)
                assert not bool(gy.untouched().any())
                close(y, want, 2e-5, 3e-5, what)
                outs.append(G.dense(y))
            if len(outs) == 2:
                assert G.same_bits(outs[0], outs[1]), what + ": fragment order differs from row-major"


@pytest.mark.parametrize("K", [512, 1024])
def test_dual_launch_is_the_two_single_launches(K):
    """two problems of unequal shape in one launch (4 / 8 waves: the paired forms), both orders, row-major and fragment order"""
    torch, F, ops, _lib = _t()
    from m3asr.plan import pack_wfrag
    lens = dev(torch.tensor([37], dtype=torch.int32))
    for frag in (False, True):
        probs = []
        for i, (M, N) in enumerate([(50, 48), (17, 32)]):
            a, w, b, res = dev(rnd(M, K, seed=10 + i)), dev(rnd(N, K, seed=20 + i, scale=K ** -0.5)), dev(rnd(N, seed=30 + i)), dev(rnd(M, N, seed=40 + i))
            probs.append(dict(a=a, w=pack_wfrag(w) if frag else w, bias=b, act=_lib.ACT_SILU, alpha=0.5, resid=res, lens=lens, rows_per_batch=64,
                              mask_out=True))
        singles = [ops.linear(**p) for p in probs]
        for order in ((0, 1), (1, 0)):
            assert ops.linear_pair_kernel(probs[order[0]], probs[order[1]]) is not None, "the pair is refused"
            ya, yb = ops.linear_pair(dict(probs[order[0]]), dict(probs[order[1]]))
            assert same(ya, singles[order[0]]) and same(yb, singles[order[1]]), "K=%d frag=%s order=%s" % (K, frag, order)


# ================================================================================================ router and engine (child processes)
MODELS = {
    "a": dict(output_dim=16, attention_dim=256, attention_heads=4, num_blocks=2, embed_heads=4, embed_dim=256, embed_linear_units=256,
              embed_blocks=1, num_experts=8, hidden_units=256),
    "b": dict(output_dim=16, attention_dim=512, attention_heads=8, num_blocks=2, embed_heads=8, embed_dim=512, embed_linear_units=256,
              embed_blocks=1, num_experts=32, hidden_units=256),
}
ROUTER_CASES = [(m, f) for m in ("a", "b") for f in (72, 100)]     # 72 frames = 17 rows (one live row in the second tile), 100 frames = 24 rows


def _child(out_path):
    """block 0 up to and including its router, for every router case (the switch M3_ROUTER_PREFIX is read once per process)"""
    import torch
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    arrays = {}
    for model in MODELS:
        cfg = EncoderConfig(**MODELS[model])
        w = make_weights(cfg, seed=5)
        eng = Engine.from_state_dict(cfg, w)
        for m, frames in ROUTER_CASES:
            if m != model:
                continue
            feat = torch.randn(1, frames, cfg.input_dim, generator=torch.Generator().manual_seed(11)).cuda()
            eng.bind(feat, torch.tensor([[frames]], dtype=torch.int32).cuda())
            names = eng.stage_names()
            at = names.index("blocks.0.moe_router")
            eng.run_stages(0, at + 1)
            torch.cuda.synchronize()
            key = "%s%d." % (m, frames)
            S = eng.buffer("x").numel() // cfg.attention_dim
            arrays[key + "x"] = eng.buffer("x").cpu().numpy().reshape(S, -1).copy()
            arrays[key + "xn"] = eng.buffer("xn").cpu().numpy().reshape(S, -1).copy()
            arrays[key + "rl"] = eng.buffer("router_logits").cpu().numpy().reshape(S, -1).copy()
            arrays[key + "gamma"] = eng.weights["blocks.0.norm_ff.weight"].cpu().numpy()
            arrays[key + "beta"] = eng.weights["blocks.0.norm_ff.bias"].cpu().numpy()
            arrays[key + "prefix"] = np.asarray(["router_e_prefix" in names])
    np.savez(out_path, **arrays)


@pytest.fixture(scope="module")
def router_runs(tmp_path_factory):
    base = {k: v for k, v in os.environ.items() if not k.startswith("M3_")}
    out = {}
    for name, env in (("on", {}), ("off", {"M3_ROUTER_PREFIX": "0"})):
        path = str(tmp_path_factory.mktemp("gemmchain") / (name + ".npz"))
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", path],
                           env=dict(base, **env), cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 0, "child %s exited with %d:\n%s" % (name, p.returncode, p.stderr[-4000:])
        out[name] = dict(np.load(path))
    return out


@pytest.mark.parametrize("model,frames", ROUTER_CASES)
def test_router_with_the_prefix_is_the_router_without(router_runs, model, frames):
    """concat + LayerNorm prologue, with acc_init and without: logits and xn bit for bit; xn against F.layer_norm at the bound
    tests/test_kernels_gpu.py::test_linear_concat_router has (2e-5 relative, 1e-4 absolute)"""
    import torch
    import torch.nn.functional as F
    on, off = router_runs["on"], router_runs["off"]
    key = "%s%d." % (model, frames)
    assert bool(on[key + "prefix"][0]) and not bool(off[key + "prefix"][0])
    S = {72: 17, 100: 24}[frames]
    assert on[key + "xn"].shape[0] == S
    for buf in ("x", "xn", "rl"):
        assert np.isfinite(on[key + buf]).all()
        assert np.array_equal(on[key + buf], off[key + buf]), key + buf
    x = torch.from_numpy(on[key + "x"]).double()
    D = x.shape[1]
    want = F.layer_norm(x, (D,), torch.from_numpy(on[key + "gamma"]).double(), torch.from_numpy(on[key + "beta"]).double(), 1e-12)
    close(torch.from_numpy(on[key + "xn"]), want, 2e-5, 1e-4, key + "xn")


ENGINE_CASES = [("tiny", [40, 29], False), ("tiny", [40, 29], None), ("b", [100, 70], False), ("b", [100, 70], None), ("b", [100], None)]


@pytest.mark.parametrize("model,lengths,packed", ENGINE_CASES)
def test_engine_eager_is_the_replayed_graph(model, lengths, packed):
    """a ragged pair on padded rows (input- and output-masked rows inside the batch: the general mask) and on packed rows
    (rows_per_batch = the row count: the one-run mask, m_dev), and one utterance: logits, gate_idx, gate_value"""
    import torch
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig.tiny() if model == "tiny" else EncoderConfig(**MODELS[model])
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=5), packed_rows=packed)
    B, T = len(lengths), max(lengths)
    feat = torch.randn(B, T, cfg.input_dim, generator=torch.Generator().manual_seed(11)).cuda()
    logits = eng.bind(feat, torch.tensor([lengths], dtype=torch.int32).cuda())

    def taps():
        torch.cuda.synchronize()
        out = [logits.cpu().numpy().copy()]
        for i in range(cfg.num_blocks):
            out.append(eng.buffer("blocks.%d.gate_idx" % i, torch.int32).cpu().numpy().copy())
            out.append(eng.buffer("blocks.%d.gate_value" % i).cpu().numpy().copy())
        return out

    eng.forward(use_graph=False)
    eager = taps()
    for _ in range(3):                 # capture, then two replays
        eng.forward(use_graph=True)
    graph = taps()
    assert all(np.isfinite(a).all() for a in eager)
    for a, b in zip(eager, graph):
        assert np.array_equal(a, b)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: test_gemm_chain_gpu.py --child OUT.npz")
