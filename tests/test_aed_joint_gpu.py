"""Joint CTC/attention decoding on the device (m3asr.aed_search with ctc_weight > 0, csrc/aed_joint.hip) against
tests/aed_joint_ref.py.

Yardstick, that of tests/test_aed_search_gpu.py: aed_joint_ref in float64 is the truth; e32 is the largest difference between
its key / att / ctc and the same quantities of the SAME kept candidates recomputed in float32 on the CPU (attention teacher-forced
through aed_search_ref.teacher_forced_scores, the CTC part by the restatement's scorer run in float32 over the kept token
lists); the device must be within max(8 e32, 1e-5) on all three.  The discrete results must be IDENTICAL for every utterance
whose float64 decision margin exceeds twice that bound; the seeds of tests/aed_joint_cases.py were picked on the CPU so that
every utterance of every case does (asserted, never skipped).  No bound comes from the device's output; every test prints the
device error, e32, the bound and the margin before it asserts (run with -s)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_joint_cases as cases
import aed_joint_ref as ref
import aed_search_ref
from m3asr import _lib
from m3asr.plan import pack_decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _searcher(name, B=None, **kw):
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, ctc, spec = cases.case(name)
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    kw.setdefault("ctc_weight", spec["w"])
    kw.setdefault("pre_beam", spec["pre_beam"])
    return AttentionBeamSearch(res, len(mem_len) if B is None else B, spec["beam"], spec["max_steps"] or max(mem_len), **kw)


def _gap(a, b):
    return 0.0 if a == b else abs(a - b)            # -inf against -inf is exact; against anything else the gap is inf


def _err(hyps, want):
    """largest difference over key, att and ctc; hyps: (tokens, key, finished, att, ctc), want: rows of (key, att, ctc)"""
    return max(max(_gap(h[1], w[0]), _gap(h[3], w[1]), _gap(h[4], w[2])) for h, w in zip(hyps, want))


def _compare(tag, out, r64, e32, bound):
    """out: search(detail=True)'s result for the utterances of r64"""
    for b, ((best, hyps), want) in enumerate(zip(out, r64)):
        err = _err(hyps, [(w[1], w[2], w[3]) for w in want["nbest"]])
        print("aed joint %s utterance %d: device err %.3e, e32 %.3e, bound %.3e, margin %.3e, steps %d / limit %d" % (
            tag, b, err, e32, bound, want["margin"], want["steps"], want["limit"]))
        assert want["margin"] > 2 * bound, "the seed leaves utterance %d with a near tie" % b
        assert [h[0] for h in hyps] == [w[0] for w in want["nbest"]]
        assert [h[2] for h in hyps] == [w[4] for w in want["nbest"]]
        assert tuple(best) == want["nbest"][want["best"]][0]
        assert not any(np.isnan(v) for h in hyps for v in (h[1], h[3], h[4])) and err <= bound, (err, bound)


def _search(s, name, **kw):
    dcfg, sd, memory, mem_len, ctc, spec = cases.case(name)
    return s.search(memory.cuda(), torch.tensor(mem_len, dtype=torch.int32), ctc_logits=ctc.cuda(), ctc_log_probs=True, **kw)


def _check(name):
    r64, e32, bound = cases.reference(name)
    s = _searcher(name)
    out = _search(s, name, detail=True)
    _compare(name, out, r64, e32, bound)
    last = {k: v.cpu() for k, v in s.last.items()}
    assert last["steps"].tolist() == [r["steps"] for r in r64] and last["done"].tolist() == [1] * len(r64)
    assert last["best"].tolist() == [r["best"] for r in r64]
    assert s.launches_per_step() == 8 * cases.case(name)[0].num_blocks + 4
    assert _search(s, name) == [list(r["nbest"][r["best"]][0]) for r in r64]      # a second call, without detail
    return r64


def test_tiny_model():
    """2 blocks, D 32, dk 16, V 11, beam 3, P 5; memories of 5, 9 and 1 frames in one call: unequal limits, m = 1 (the
    recursion's empty range), an utterance that hits its limit with live slots, a kept candidate whose token repeats its
    parent's last token (the c == last branch), and a kept -inf key"""
    r64 = _check("tiny")
    eos = cases.case("tiny")[0].vocab - 1
    assert [r["limit"] for r in r64] == [5, 9, 1]
    assert any(cases.hits_limit_unfinished(r) for r in r64[:2])
    assert any(cases.repeat_steps(r, eos) for r in r64)
    assert any(cases.minus_inf_steps(r) for r in r64)


def test_scorer_state_follows_the_hypotheses():
    """the parts and tokens after 1, 2, .. k steps (max_steps = 1 .. k) against the float64 history, across a step whose kept
    candidates share a parent while another parent has none and a later step that extends them: the scorer state must follow
    the parents, not the slots"""
    dcfg, sd, memory, mem_len, ctc, spec = cases.case("tiny")
    r64, e32, bound = cases.reference("tiny")
    b = max(range(len(r64)), key=lambda i: len(cases.ancestry_steps(r64[i])))
    hist = r64[b]["history"]
    assert cases.ancestry_steps(r64[b]) and min(cases.ancestry_steps(r64[b])) < len(hist) and r64[b]["margin"] > 2 * bound
    s = _searcher("tiny")
    eos = dcfg.vocab - 1
    for k in range(1, len(hist) + 1):
        _, hyps = _search(s, "tiny", detail=True, max_steps=k)[b]
        entry = hist[k - 1]
        err = _err(hyps, list(zip(entry["key"].tolist(), entry["att"].tolist(), entry["ctc"].tolist())))
        print("aed joint history: %d steps, parents %s, device err %.3e, bound %.3e" % (k, entry["parent"], err, bound))
        assert [h[0] for h in hyps] == [aed_search_ref.strip(t, eos) for t in entry["tokens"]]
        assert [h[2] for h in hyps] == entry["finished"] and err <= bound


@pytest.mark.parametrize("name", ["w1_p_is_vocab", "beam1", "p_is_beam", "p64"])
def test_weights_and_pre_beams(name):
    """w = 1 with P = V = 5 (attention only proposes), beam 1, P = N, and P = 64 of V = 70"""
    r64 = _check(name)
    spec = cases.case(name)[5]
    if name == "w1_p_is_vocab":
        assert spec["w"] == 1.0 and spec["pre_beam"] == spec["dcfg"].vocab == 5
        for r in r64:
            assert all(h[1] == h[3] for h in r["nbest"])                      # the key IS the CTC part
    if name == "p64":
        assert spec["pre_beam"] == 64 and spec["dcfg"].vocab == 70


def test_frame_tiles():
    """memories of 63, 64, 65 and 130 frames: the edges of the 64-frame tile of the parent's state, of the 16-frame tile of the
    gathered operand, and more than two tiles"""
    r64 = _check("frames")
    assert [r["limit"] for r in r64] == [6, 6, 6, 6] and cases.case("frames")[3] == [63, 64, 65, 130]


def test_real_widths_one_block():
    """D 512 / F 2048 / V 1434 / dk 128, one block, beam 4, P 6, memories of 70 and 37 frames, 12 steps"""
    r64 = _check("real")
    assert all(r["limit"] == 12 for r in r64)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_row_independence():
    """an utterance searched alone and inside a batch of three: the same bits in tokens and all three scores"""
    dcfg, sd, memory, mem_len, ctc, spec = cases.case("tiny")
    batch, alone = _searcher("tiny"), _searcher("tiny", B=1)
    _search(batch, "tiny")
    full = {k: v.cpu() for k, v in batch.last.items()}
    for b in range(3):
        alone.search(memory[b:b + 1].cuda(), mem_len[b:b + 1], ctc_logits=ctc[b:b + 1].cuda(), ctc_log_probs=True)
        for key in ("score", "att", "ctc", "hyp_tokens", "hyp_len", "finished", "best", "steps"):
            assert torch.equal(_bits(alone.last[key].cpu()), _bits(full[key][b:b + 1])), (key, b)


@pytest.mark.parametrize("name", ["w1_p_is_vocab", "beam1"])
def test_frozen_utterances(name):
    """steps issued past an utterance's end are no-ops: polling every step and every 8 steps leave the same bits in the results
    and in BOTH state blobs.  The cases are those whose utterances all end before the largest limit, so that poll = 8 does
    issue steps that poll = 1 does not."""
    a, b = _searcher(name, poll=1), _searcher(name, poll=8)
    ra, rb = _search(a, name, detail=True), _search(b, name, detail=True)
    r64 = cases.reference(name)[0]
    print("aed joint frozen %s: %d steps issued with poll = 1, %d with poll = 8, the utterances took %s" % (
        name, a.steps_issued, b.steps_issued, [r["steps"] for r in r64]))
    assert a.steps_issued == max(r["steps"] for r in r64) < b.steps_issued
    assert ra == rb
    assert torch.equal(a.last["state"].cpu(), b.last["state"].cpu())
    assert torch.equal(a.last["joint_state"].cpu(), b.last["joint_state"].cpu())
    for key in ("score", "att", "ctc", "hyp_tokens", "finished", "steps"):
        assert torch.equal(_bits(a.last[key].cpu()), _bits(b.last[key].cpu())), key


def test_packed_rows_equal_the_padded_layout():
    dcfg, sd, memory, mem_len, ctc, spec = cases.case("tiny")
    padded, packed = _searcher("tiny"), _searcher("tiny")
    want = padded.search(memory.cuda(), mem_len, ctc_logits=ctc.cuda(), ctc_log_probs=True, detail=True)
    rows = torch.cat([memory[b, :m] for b, m in enumerate(mem_len)]).cuda()
    crow = torch.cat([ctc[b, :m] for b, m in enumerate(mem_len)]).cuda()
    row0 = torch.tensor([0] + list(np.cumsum(mem_len)), dtype=torch.int32)
    got = packed.search_rows(rows, row0, raw_memory=False, ctc_rows=crow, ctc_log_probs=True, detail=True)
    assert got == want
    for key in ("score", "att", "ctc", "hyp_tokens", "finished", "steps"):
        assert torch.equal(_bits(packed.last[key].cpu()), _bits(padded.last[key].cpu())), key


def test_graph_option_gives_the_same_bits():
    eager, graph = _searcher("tiny"), _searcher("tiny", use_graph=True)
    want = _search(eager, "tiny", detail=True)
    for _ in range(2):                                            # the capturing call and a replaying one
        assert _search(graph, "tiny", detail=True) == want
        assert torch.equal(graph.last["state"].cpu(), eager.last["state"].cpu())
        assert torch.equal(graph.last["joint_state"].cpu(), eager.last["joint_state"].cpu())
        for key in ("score", "att", "ctc"):
            assert torch.equal(_bits(graph.last[key].cpu()), _bits(eager.last[key].cpu())), key


def test_device_log_softmax_of_logits():
    """the public path: raw CTC logits, log-softmax on the device (m3_log_softmax_bias), against log-probabilities made on the
    CPU from the same logits.  The yardstick holds; bits may differ in the last place of the log-softmax."""
    dcfg, sd, memory, mem_len, ctc, spec = cases.case("tiny")
    r64, e32, bound = cases.reference("tiny")
    s = _searcher("tiny")
    out = s.search(memory.cuda(), mem_len, ctc_logits=(ctc + 3.0).cuda(), detail=True)      # log_softmax(x + c) = log_softmax(x)
    _compare("device log-softmax", out, r64, e32, bound)


def test_ctc_weight_zero_is_the_search_of_before():
    """ctc_weight = 0: no scorer state, 8 L + 3 launches, the same bits as an AttentionBeamSearch built without the keyword"""
    from m3asr.aed_search import AttentionBeamSearch
    dcfg, sd, memory, mem_len, ctc, spec = cases.case("tiny")
    zero = _searcher("tiny", ctc_weight=0.0, pre_beam=None)
    plain = AttentionBeamSearch(zero.rescorer, len(mem_len), spec["beam"], max(mem_len))
    a = zero.search(memory.cuda(), mem_len, detail=True)
    b = plain.search(memory.cuda(), mem_len, detail=True)
    assert a == b and all(len(h) == 3 for _, hyps in a for h in hyps)
    assert zero.jstate is None and zero.jscratch is None and zero.jdesc is None and zero.ctc is None
    assert zero.launches_per_step() == plain.launches_per_step() == 8 * dcfg.num_blocks + 3
    assert "att" not in zero.last and "joint_state" not in zero.last
    assert torch.equal(zero.last["state"].cpu(), plain.last["state"].cpu())
    assert torch.equal(_bits(zero.last["score"].cpu()), _bits(plain.last["score"].cpu()))


def test_refusals():
    """a weight outside [0, 1], P < N, P > 64, P > V, a CTC vocabulary != V, CTC frames fewer than the memory's, missing and
    unexpected CTC input: M3Error before any launch"""
    from m3asr import ops
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, ctc, spec = cases.case("tiny")
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    for w in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.M3Error, match="ctc_weight"):
            AttentionBeamSearch(res, 3, 3, 9, ctc_weight=w)
    for p in (2, 65, 12):                                        # beam 3, V 11
        with pytest.raises(_lib.M3Error, match="pre_beam"):
            AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5, pre_beam=p)
    big = cases.case("p64")[0]                                   # V 70: P = 65 fits the vocabulary, not the wave
    with pytest.raises(_lib.M3Error, match="pre_beam"):
        AttentionBeamSearch(AttentionRescorer(pack_decoder(cases.case("p64")[1], big), big, "cuda:0"), 1, 3, 4, ctc_weight=0.5, pre_beam=65)
    sdesc = ops.aed_search_desc(3, 3, 9, 11, 32, 2, 2, 100)
    for p, frames, what in ((2, 9, "pre_beam"), (65, 9, "pre_beam"), (12, 9, "pre_beam"), (5, 0, "max_frames"), (5, 1 << 21, "max_frames")):
        with pytest.raises(_lib.M3Error, match=what):
            ops.aed_joint_desc(sdesc, p, frames)
    with pytest.raises(_lib.M3Error, match="overflow"):
        ops.aed_joint_desc(ops.aed_search_desc(4096, 64, 16, 1434, 512, 4, 1, 100), 64, 1 << 16)
    assert AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5).pre_beam == 5        # min(max(3, ceil(4.5)), 64, 11)
    s = AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5, pre_beam=5)
    mem, lens = memory.cuda(), mem_len
    with pytest.raises(_lib.M3Error, match="needs the CTC output"):
        s.search(mem, lens)
    with pytest.raises(_lib.M3Error, match="classes"):
        s.search(mem, lens, ctc_logits=torch.zeros(3, 9, 12))
    with pytest.raises(_lib.M3Error, match="frames"):
        s.search(mem, lens, ctc_logits=ctc[:, :8].cuda())
    rows = torch.cat([memory[b, :m] for b, m in enumerate(mem_len)]).cuda()
    row0 = torch.tensor([0, 5, 14, 15], dtype=torch.int32)
    with pytest.raises(_lib.M3Error, match="frames"):
        s.search_rows(rows, row0, raw_memory=False, ctc_rows=torch.zeros(14, 11))
    with pytest.raises(_lib.M3Error, match="needs the CTC output"):
        s.search_rows(rows, row0, raw_memory=False)
    assert s.last is None and s.steps_issued == 0 and s.jstate is None
    z = AttentionBeamSearch(res, 3, 3, 9)
    with pytest.raises(_lib.M3Error, match="ctc_weight = 0"):
        z.search(mem, lens, ctc_logits=ctc.cuda())
    assert z.last is None and z.steps_issued == 0


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_end_to_end_builder_and_infer(tmp_path):
    """synthetic CTC/attention checkpoint -> builder.py -> infer.py --attention --ctc-weight 0.3 prints what
    CtcDecoder.attention(ctc_weight=0.3) returns, both parts included; and that is what aed_joint_ref finds on Engine.hidden()
    and the forward's own logits"""
    from m3asr.decode import CtcDecoder
    from m3asr.engine import Engine
    from m3asr.plan import decoder_config_of, load_plan
    from m3asr.rescore import AttentionRescorer
    d = str(tmp_path)
    beam, steps, w = 3, 6, 0.3
    _run(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--decoder-blocks", "2", "--seed", "4"])
    model = os.path.join(d, "model.pt")
    sd = torch.load(model, map_location="cpu", weights_only=True)
    plan = os.path.join(d, "aed.plan")
    _run(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", model, "-o", plan, "--opt-shape", "2x80"])
    g = torch.Generator().manual_seed(7)
    feat = torch.rand(2, 90, 40, generator=g)
    np.save(os.path.join(d, "feat.npy"), feat.numpy())
    printed = _run(["infer.py", "-p", plan, "-i", os.path.join(d, "feat.npy"), "--attention", "--beam", str(beam), "--max-steps", str(steps),
                    "--ctc-weight", str(w)])
    shown = {int(m.group(1)): (float(m.group(2)), float(m.group(3)), float(m.group(4)), [int(t) for t in m.group(5).split()])
             for m in re.finditer(r"^utt (\d+) attention: score=(\S+) att=(\S+) ctc=(\S+) finished=\d tokens=([\d ]*)$", printed, re.M)}
    assert sorted(shown) == [0, 1], printed[-2000:]

    cfg, packed, extra = load_plan(plan)
    dcfg = decoder_config_of(extra)
    eng = Engine(cfg, packed, device="cuda:0")
    dec = CtcDecoder(eng, rescorer=AttentionRescorer(packed, dcfg, "cuda:0"))
    lens = torch.full((2,), feat.shape[1], dtype=torch.int32)
    detail = dec.attention(feat, lens, beam, max_steps=steps, detail=True, ctc_weight=w)
    assert [u[0] for u in detail] == [shown[0][3], shown[1][3]] == dec.attention(feat, lens, beam, max_steps=steps, ctc_weight=w)
    for b, (best, hyps) in enumerate(detail):
        chosen = next(h for h in hyps if list(h[0]) == best)
        assert ["%.4f" % v for v in (chosen[1], chosen[3], chosen[4])] == ["%.4f" % v for v in shown[b][:3]]
    hidden = eng.hidden().cpu()
    out_lens = eng.buffer("lens", torch.int32)[:2].cpu().tolist()
    logits = dec.forward(feat, lens)["out_nosm"].cpu()
    ctc = torch.log_softmax(logits.double(), dim=-1)
    w32 = float(np.float32(w))                                   # the C ABI takes the weight as a float
    r64 = ref.search(sd, dcfg, hidden, out_lens, ctc, beam, min(max(beam, -(-3 * beam // 2)), 64, dcfg.vocab), w32, steps, dtype=torch.float64)
    e32 = ref.e32_of(r64, ref.recomputed_parts(sd, dcfg, hidden, out_lens, ctc.float(), r64, w32, dtype=torch.float32))
    _compare("end to end", detail, r64, e32, max(8 * e32, 1e-5))
