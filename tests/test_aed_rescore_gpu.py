"""Attention rescoring on the device (m3asr.rescore, csrc/aed_rescore.hip) against tests/aed_ref.py.

Yardstick, as tests/test_fbank_gpu.py: aed_ref in float64 is the truth; e32 is the error of the SAME aed_ref evaluated in
float32 on the CPU for the test's own inputs (another correct fp32 evaluation order); the device must be within
max(8 e32, 1e-5) of float64.  No bound comes from the device's output; every test prints its error, e32 and the bound before
it asserts (run with -s).  The chosen hypothesis is compared where the float64 reference's two best final scores lie more
than twice the bound apart; the seeds below were picked on the CPU so that every utterance does (asserted, never skipped)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_ref
from m3asr import _lib
from m3asr.config import DecoderConfig, EncoderConfig
from m3asr.plan import pack_decoder, pack_weights, memory_norm
from m3asr.weights import make_decoder_weights, make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nbest_tensors(hyps, beam, max_frames):
    """[[(tokens, prior)]] per utterance -> (hyp_tokens, hyp_len, hyp_score, n_hyps) as m3_ctc_beam_nbest leaves them; the
    slots past an utterance's n-best hold a stale length, which the rescorer must not look at"""
    B = len(hyps)
    toks = torch.full((B, beam, max_frames), -1, dtype=torch.int32)
    hlen = torch.full((B, beam), 5, dtype=torch.int32)
    score = torch.full((B, beam), -float("inf"))
    n = torch.tensor([len(h) for h in hyps], dtype=torch.int32)
    for b, hs in enumerate(hyps):
        for i, (y, prior) in enumerate(hs):
            toks[b, i, :len(y)] = torch.tensor(y, dtype=torch.int32)
            hlen[b, i] = len(y)
            score[b, i] = prior
    return toks, hlen, score, n


@functools.lru_cache(maxsize=None)
def _case(name):
    """(dcfg, state dict, memory (B,T,D), mem_len, hyps) of a named test case; the random draws depend on the name only"""
    tiny = dict(lens=([9, 0, 1], [4, 4]), mem=(11, 7), beam=3)
    spec = {
        "tiny": dict(dcfg=DecoderConfig.tiny(), seed=11, **tiny),
        "tiny_bi": dict(dcfg=DecoderConfig.tiny(r_num_blocks=1), seed=12, **tiny),
        "real_h4": dict(dcfg=DecoderConfig(vocab=1434, dim=512, heads=4, linear_units=2048, num_blocks=1), seed=13,
                        lens=([20, 20, 20, 20], [7, 7, 7, 7]), mem=(130, 37), beam=4),
        "real_h8": dict(dcfg=DecoderConfig(vocab=1434, dim=512, heads=8, linear_units=2048, num_blocks=1), seed=14,
                        lens=([20, 20, 20, 20], [7, 7, 7, 7]), mem=(130, 37), beam=4),
    }[name]
    dcfg = spec["dcfg"]
    g = torch.Generator().manual_seed(spec["seed"])
    sd = make_decoder_weights(dcfg, seed=spec["seed"])
    sd["after_norm.weight"] = torch.rand(dcfg.dim, generator=g) + 0.5       # the encoder's, for pack_decoder
    sd["after_norm.bias"] = torch.randn(dcfg.dim, generator=g) * 0.1
    mem_len = list(spec["mem"])
    memory = torch.randn(len(mem_len), max(mem_len), dcfg.dim, generator=g)  # frames past mem_len: live numbers, to be masked
    hyps = [[(tuple(torch.randint(0, dcfg.vocab - 1, (n,), generator=g).tolist()), float(-torch.rand((), generator=g) * 10 - 1))
             for n in lens] for lens in spec["lens"]]
    return dcfg, sd, memory, mem_len, hyps, spec["beam"]


@functools.lru_cache(maxsize=None)
def _reference(name, ctc_weight, reverse_weight):
    """(float64 result, float32 result) of aed_ref on the case: computed once, shared by the tests"""
    dcfg, sd, memory, mem_len, hyps, _ = _case(name)
    return tuple(aed_ref.rescore(sd, dcfg, memory, mem_len, hyps, ctc_weight, reverse_weight, dtype=dt)
                 for dt in (torch.float64, torch.float32))


def _yardstick(r64, r32, key):
    e32 = max(abs(a - b) for u64, u32 in zip(r64, r32) for a, b in zip(u64[key], u32[key]))
    return e32, max(8 * e32, 1e-5)


def _top_two_gap(final):
    s = sorted(final, reverse=True)
    return float("inf") if len(s) < 2 else s[0] - s[1]


def _device(name, ctc_weight=0.0, reverse_weight=0.0, max_frames=24):
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, hyps, beam = _case(name)
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    tensors = tuple(t.cuda() for t in _nbest_tensors(hyps, beam, max_frames))
    out = res.rescore(memory.cuda(), torch.tensor(mem_len, dtype=torch.int32), tensors, ctc_weight=ctc_weight,
                      reverse_weight=reverse_weight)
    return out, {k: v.cpu() for k, v in res.last.items()}, hyps, beam


def _check(name, ctc_weight=0.0, reverse_weight=0.0, keys=("att",)):
    out, last, hyps, beam = _device(name, ctc_weight, reverse_weight)
    r64, r32 = _reference(name, ctc_weight, reverse_weight)
    for key in keys:
        e32, bound = _yardstick(r64, r32, key)
        err = max(abs(float(last[key][b, i]) - v) for b, u in enumerate(r64) for i, v in enumerate(u[key]))
        print("aed %s %s: device err %.3e, e32 %.3e, bound %.3e" % (name, key, err, e32, bound))
        assert all(np.isfinite(float(last[key][b, i])) for b, u in enumerate(r64) for i in range(len(u[key])))
        assert err <= bound, (key, err, bound)
    _, fbound = _yardstick(r64, r32, "final")
    for b, u in enumerate(r64):
        n = len(hyps[b])
        gap = _top_two_gap(u["final"])
        print("aed %s utterance %d: reference top-two final gap %.3e (2 x bound %.3e), best %d" % (name, b, gap, 2 * fbound, u["best"]))
        assert gap > 2 * fbound, "the seed leaves utterance %d without a decided winner" % b
        assert int(last["best"][b]) == u["best"]
        assert list(out[b][0]) == list(hyps[b][u["best"]][0]) and len(out[b][1]) == n
        assert [h[0] for h in out[b][1]] == [h[0] for h in hyps[b]]
        for key in ("att", "r_att", "final"):                 # dead slots are reported as such
            assert bool(torch.isneginf(last[key][b, n:]).all()), (key, b)
    return last


def test_tiny_model():
    """D = 32, dk = 16, 2 blocks; hypotheses of 0, 1 and 9 tokens, memory lengths (11, 7), one utterance with 2 < beam"""
    _check("tiny")


@pytest.mark.parametrize("name", ["real_h4", "real_h8"])
def test_real_dimensions_one_block(name):
    """D = 512, F = 2048, V = 1434 with dk = 128 and dk = 64; 130 keys cross the kernel's key tiles, 37 is no multiple of 16"""
    _check(name)


def test_right_to_left_decoder():
    last = _check("tiny_bi", ctc_weight=0.5, reverse_weight=0.3, keys=("att", "r_att", "final"))
    assert float(last["r_att"][0, 0]) != 0.0


def test_row_independence():
    """the same utterance and hypotheses at b = 0 and b = 2 of one batch give the same bits"""
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, hyps, beam = _case("tiny_bi")
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    mem3 = torch.stack([memory[0], memory[1], memory[0]])
    tensors = tuple(t.cuda() for t in _nbest_tensors([hyps[0], hyps[1], hyps[0]], beam, 24))
    out = res.rescore(mem3.cuda(), torch.tensor([mem_len[0], mem_len[1], mem_len[0]], dtype=torch.int32), tensors,
                      ctc_weight=0.5, reverse_weight=0.3)
    for key in ("att", "r_att", "final"):
        t = res.last[key].cpu()
        assert torch.isfinite(t[0]).all() and torch.equal(t[0], t[2]), key
    assert out[0] == out[2] and int(res.last["best"][0]) == int(res.last["best"][2])


def test_rejects_what_it_cannot_score():
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, hyps, beam = _case("tiny")
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    tensors = tuple(t.cuda() for t in _nbest_tensors(hyps, beam, 24))
    with pytest.raises(_lib.M3Error, match="kv_len = 0"):
        res.rescore(memory.cuda(), torch.tensor([11, 0], dtype=torch.int32), tensors)
    with pytest.raises(_lib.M3Error, match="right-to-left"):
        res.rescore(memory.cuda(), torch.tensor(mem_len, dtype=torch.int32), tensors, reverse_weight=0.3)
    # an utterance whose search failed (n_hyps = -1) has no hypotheses and needs no memory
    toks, hlen, score, n = tensors
    out = res.rescore(memory.cuda(), torch.tensor([11, 0], dtype=torch.int32), (toks, hlen, score, torch.tensor([3, -1], dtype=torch.int32).cuda()))
    assert out[1] == ((), []) and int(res.last["best"][1]) == -1 and len(out[0][1]) == 3


@pytest.mark.parametrize("ragged", [False, True])
def test_engine_hidden(golden, ragged):
    """Engine.hidden() is the input of out_linear: hidden @ W_out^T + b in float64 from the unfolded weights matches the engine's
    logits (which come from the folded GEMM on the residual stream), for padded rows and for packed rows"""
    from m3asr.engine import Engine
    cfg, z = golden("tiny")
    w = make_weights(cfg, seed=int(z["weight_seed"]))
    packed = pack_weights(w, cfg)
    packed.update(memory_norm(w))
    feat = torch.from_numpy(z["feat"])[:2].contiguous()
    T = feat.shape[1]
    lens = torch.tensor([[T, T - 11 if ragged else T]], dtype=torch.int32)
    eng = Engine(cfg, packed, device="cuda:0", packed_rows=ragged)
    logits = eng(feat.cuda(), lens.cuda()).cpu()
    assert eng.packed_rows() == ragged
    hidden = eng.hidden().cpu()
    raw = eng.hidden(normalized=False).cpu()
    out_lens = eng.buffer("lens", torch.int32)[:2].cpu().tolist()
    assert tuple(hidden.shape) == (2, logits.shape[1], cfg.attention_dim)
    W, b = w["out_linear.weight"], w["out_linear.bias"]
    err = e32 = 0.0
    for u, n in enumerate(out_lens):
        want = hidden[u, :n].double() @ W.double().t() + b.double()
        e32 = max(e32, float(((hidden[u, :n] @ W.t() + b).double() - want).abs().max()))
        err = max(err, float((logits[u, :n].double() - want).abs().max()))
        ln = aed_ref.layer_norm(raw[u, :n].double(), w["after_norm.weight"].double(), w["after_norm.bias"].double())
        assert float((hidden[u, :n].double() - ln).abs().max()) <= 1e-5
    bound = max(8 * e32, 1e-5)
    print("engine hidden (ragged=%s): logits err %.3e, e32 %.3e, bound %.3e" % (ragged, err, e32, bound))
    assert err <= bound, (err, bound)
    # without the vectors in its plan the engine says so
    with pytest.raises(_lib.M3Error, match="after_norm"):
        e2 = Engine(cfg, pack_weights(w, cfg), device="cuda:0")
        e2(feat.cuda(), lens.cuda())
        e2.hidden()


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_end_to_end_builder_and_infer(tmp_path):
    """synthetic CTC/attention checkpoint -> builder.py -> infer.py --rescore prints the hypothesis that
    CtcDecoder.attention_rescoring returns, which is the one aed_ref picks on Engine.hidden() and the same n-best"""
    from m3asr.decode import CtcBeamSearch, CtcDecoder
    from m3asr.engine import Engine
    from m3asr.plan import decoder_config_of, load_plan
    from m3asr.rescore import AttentionRescorer
    d = str(tmp_path)
    beam, cw = 4, 0.3
    _run(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--decoder-blocks", "2", "--seed", "4"])
    plan = os.path.join(d, "aed.plan")
    _run(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", os.path.join(d, "model.pt"), "-o", plan, "--opt-shape", "2x80"])
    g = torch.Generator().manual_seed(7)
    feat = torch.rand(2, 90, 40, generator=g)
    np.save(os.path.join(d, "feat.npy"), feat.numpy())
    printed = _run(["infer.py", "-p", plan, "-i", os.path.join(d, "feat.npy"), "--rescore", "--beam", str(beam), "--ctc-weight", str(cw)])
    shown = {int(m.group(1)): [int(t) for t in m.group(2).split()]
             for m in re.finditer(r"^utt (\d+) rescored: .*tokens=([\d ]*)$", printed, re.M)}
    assert sorted(shown) == [0, 1], printed[-2000:]

    cfg, packed, extra = load_plan(plan)
    dcfg = decoder_config_of(extra)
    assert dcfg == DecoderConfig.tiny(num_blocks=2)
    eng = Engine(cfg, packed, device="cuda:0")
    assert not any(k.startswith("decoder.") for k in eng.weights)
    dec = CtcDecoder(eng, rescorer=AttentionRescorer(packed, dcfg, "cuda:0"))
    lens = torch.full((2,), feat.shape[1], dtype=torch.int32)
    detail = dec.attention_rescoring(feat, lens, beam, ctc_weight=cw, detail=True)
    best = dec.attention_rescoring(feat, lens, beam, ctc_weight=cw)
    assert best == [list(u[0]) for u in detail] and best == [shown[0], shown[1]]

    # the same n-best and the engine's hidden states through the float64 contract
    hidden = eng.hidden().cpu()
    out_lens = eng.buffer("lens", torch.int32)[:2].cpu().tolist()
    nbest = [[(h[0], h[1]) for h in u[1]] for u in detail]
    sd = torch.load(os.path.join(d, "model.pt"), map_location="cpu", weights_only=True)
    r64 = aed_ref.rescore(sd, dcfg, hidden, out_lens, nbest, cw, 0.0, dtype=torch.float64)
    r32 = aed_ref.rescore(sd, dcfg, hidden, out_lens, nbest, cw, 0.0, dtype=torch.float32)
    for key in ("att", "final"):
        e32, bound = _yardstick(r64, r32, key)
        err = max(abs(h[2 if key == "att" else 3] - v) for u, r in zip(detail, r64) for h, v in zip(u[1], r[key]))
        print("aed end to end %s: device err %.3e, e32 %.3e, bound %.3e" % (key, err, e32, bound))
        assert err <= bound, (key, err, bound)
    _, fbound = _yardstick(r64, r32, "final")
    for b, r in enumerate(r64):
        gap = _top_two_gap(r["final"])
        print("aed end to end utterance %d: %d hypotheses, reference top-two final gap %.3e (2 x bound %.3e)" % (
            b, len(nbest[b]), gap, 2 * fbound))
        assert len(nbest[b]) >= 2 and gap > 2 * fbound
        assert best[b] == list(nbest[b][r["best"]][0])
    # the hidden states are also what ctc_prefix_beam_search hands over on request
    hyps, hid1 = dec.ctc_prefix_beam_search(feat[:1], lens[:1], beam, return_hidden=True)
    assert tuple(hid1.shape) == (1, hidden.shape[1], cfg.attention_dim)
