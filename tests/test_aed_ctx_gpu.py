"""Attention decoding with hotword biasing on the device (m3asr.aed_search with context=, the <CTC, LM, true> instantiations of
csrc/aed_joint.hip) against tests/aed_ctx_ref.py.

Yardstick, that of tests/test_aed_joint_gpu.py, no new tolerance: aed_ctx_ref in float64 is the truth; e32 is the largest
difference between its key / att / ctc and the same quantities of the SAME kept candidates recomputed in float32 on the CPU; the
device must be within max(8 e32, 1e-5) on all three.  The device's bonus must EQUAL the float32 rounding of the reference's
double (both are the same double sums of the same float32 table entries in the same order), its ctx_state (and lm, lm_state,
token counts) must be equal, and the discrete results identical; every utterance's float64 decision margin exceeds twice the
bound (seeds picked on the CPU, tests/aed_ctx_cases.py; asserted, never skipped).  No bound comes from the device's output;
every test prints the device error, e32, the bound and the margin before it asserts (run with -s).  No case hands the kernels
an image that m3_ctc_context_validate rejects: every image is a ContextSet's, whose constructor validates it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_ctx_cases as cases
import aed_ctx_ref as ref
import aed_search_ref
from m3asr import _lib
from m3asr.context import ContextGraph, ContextSet
from m3asr.plan import pack_decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _searcher(name, B=None, ctx=True, **kw):
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, ctc, spec, lm, graphs = cases.case(name)
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    kw.setdefault("ctc_weight", spec["w"])
    kw.setdefault("pre_beam", spec["pre_beam"])
    if lm is not None:
        kw.update(lm=lm.to("cuda:0"), lm_weight=spec["alpha"], length_bonus=spec["beta"], lm_eos=spec["use_eos"])
    if ctx:
        kw.update(context=ContextSet(graphs, device="cuda:0", vocab_size=dcfg.vocab))
    return AttentionBeamSearch(res, len(mem_len) if B is None else B, spec["beam"], spec["max_steps"] or max(mem_len), **kw)


def _search(s, name, **kw):
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case(name)
    if s.ctc_weight > 0:
        kw.update(ctc_logits=ctc.cuda(), ctc_log_probs=True)
    if s.lm is not None:
        kw.setdefault("lm_on", spec["lm_on"])
    if s.context is not None:
        kw.setdefault("graph_ids", spec["ids"])
    return s.search(memory.cuda(), torch.tensor(mem_len, dtype=torch.int32), **kw)


def _gap(a, b):
    return 0.0 if a == b else abs(a - b)            # -inf against -inf is exact; against anything else the gap is inf


def _err(hyps, want):
    """largest difference over key, att and ctc; hyps: (tokens, key, finished, att, ctc, ...), want: rows of (key, att, ctc)"""
    return max(max(_gap(h[1], w[0]), _gap(h[3], w[1]), _gap(h[4], w[2])) for h, w in zip(hyps, want))


def _f32(v):
    return float(np.float32(v))


def _compare(tag, out, r64, e32, bound, with_lm):
    """out: search(detail=True)'s result for the utterances of r64; a hypothesis is (tokens, key, finished, att, ctc[, lm], bonus,
    final), the reference's (tokens, key, att, ctc, finished, lm, bonus, final)"""
    for b, ((best, hyps), want) in enumerate(zip(out, r64)):
        err = _err(hyps, [(w[1], w[2], w[3]) for w in want["nbest"]])
        print("aed ctx %s utterance %d: device err %.3e, e32 %.3e, bound %.3e, margin %.3e, steps %d / limit %d, bonus %s" % (
            tag, b, err, e32, bound, want["margin"], want["steps"], want["limit"], [h[-2] for h in hyps]))
        assert want["margin"] > 2 * bound, "the seed leaves utterance %d with a near tie" % b
        assert all(len(h) == (8 if with_lm else 7) for h in hyps)
        assert [h[0] for h in hyps] == [w[0] for w in want["nbest"]]
        assert [h[2] for h in hyps] == [w[4] for w in want["nbest"]]
        assert tuple(best) == want["nbest"][want["best"]][0]
        if with_lm:
            assert [h[5] for h in hyps] == [_f32(w[5]) for w in want["nbest"]]         # exactly
        assert [h[-2] for h in hyps] == [_f32(w[6]) for w in want["nbest"]]            # exactly
        assert [h[-1] for h in hyps] == [_f32(w[6]) - (w[6] - w[7]) for w in want["nbest"]]   # bonus - pot[ctx_state]
        assert not any(np.isnan(v) for h in hyps for v in (h[1], h[3], h[4])) and err <= bound, (err, bound)


def _check(name):
    r64, e32, bound = cases.reference(name)
    s = _searcher(name)
    out = _search(s, name, detail=True)
    _compare(name, out, r64, e32, bound, s.lm is not None)
    last = {k: v.cpu() for k, v in s.last.items()}
    assert last["steps"].tolist() == [r["steps"] for r in r64] and last["done"].tolist() == [1] * len(r64)
    assert last["best"].tolist() == [r["best"] for r in r64]
    assert last["ctx_state"].tolist() == [r["ctx_state"] for r in r64]
    if s.lm is not None:
        assert last["lm_state"].tolist() == [r["lm_state"] for r in r64] and last["lm_n"].tolist() == [r["n"] for r in r64]
    assert s.launches_per_step() == 8 * cases.case(name)[0].num_blocks + 4
    assert _search(s, name) == [list(r["nbest"][r["best"]][0]) for r in r64]      # a second call, without detail
    return r64, s


@pytest.mark.parametrize("name", ["tiny", "ctc", "lm", "att"])
def test_all_four_forms_on_the_tiny_shape(name):
    """V 11, beam 3, P 5, memories of 5 / 9 / 1 frames in one call: CTC with LM, CTC alone, LM alone (ctc_weight = 0), neither
    (ctc_weight = 0 and no LM: the <false, false, true> form, whose att part and candidate records live in the context blobs)"""
    r64, s = _check(name)
    spec = cases.case(name)[5]
    assert [r["limit"] for r in r64] == [5, 9, 1]
    assert (s.ctc_weight > 0, s.lm is not None) == {"tiny": (True, True), "ctc": (True, False), "lm": (False, True), "att": (False, False)}[name]
    assert any(h[6] != 0.0 for r in r64 for h in r["nbest"]) or any(x != 0.0 for r in r64 for x in cases.kept_bonus(r))
    if spec["w"] == 0:
        assert s.jstate is None and s.ctc is None and "joint_state" not in s.last and s.last["ctc"].abs().max().item() == 0
    if name in ("ctc", "att"):
        assert s.lstate is None and s.lm_on is None and "lm" not in s.last
    if name == "att":
        assert s.pre_beam == 5                                      # the pre-beam applies with a context alone


@pytest.mark.parametrize("name", ["beam1", "w1_p_is_vocab", "p64", "frames", "graphs"])
def test_shapes_and_graphs(name):
    """beam 1 with P 2; P = V = 5 with ctc_weight = 1; P = 64 of V = 70 (every lane gathers); memories of 63 / 64 / 65 frames
    with max_steps = 6 (the arc in front of the frame chain's tile edges, hypotheses cut at the step limit with provisional
    credit); a graph with failure links, a prefix phrase and a one-token phrase"""
    r64, s = _check(name)
    spec = cases.case(name)[5]
    if name == "beam1":
        assert spec["beam"] == 1 and spec["pre_beam"] == 2
    if name == "w1_p_is_vocab":
        assert spec["w"] == 1.0 and spec["pre_beam"] == spec["dcfg"].vocab == 5
    if name == "p64":
        assert spec["pre_beam"] == 64 and spec["dcfg"].vocab == 70
    if name == "frames":
        assert list(spec["mem"]) == [63, 64, 65] and [r["limit"] for r in r64] == [6, 6, 6]
        assert any(not h[4] and h[6] != h[7] for r in r64 for h in r["nbest"])          # provisional credit at the limit


def test_real_widths_one_block():
    """D 512 / F 2048 / V 1434 / dk 128, one block, beam 4, P 6, memories of 70 and 37 frames, 12 steps, a graph of 50 phrases"""
    r64, _ = _check("real")
    assert all(r["limit"] == 12 for r in r64) and len(cases.case("real")[7][0].phrases) == 50


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _utterance_words(s, blob, u):
    """the int32 words of utterance u in a state blob of searcher s: its header and both records of its rows, or its rows of the
    scorer state / the LM state"""
    N, B = s.beam, s.B
    w = s.last[blob].cpu().view(torch.int32)
    if blob == "state":
        rec = 2 * (2 + 2 * (s.max_steps + 1))
        return torch.cat([w[u * 8:(u + 1) * 8], w[B * 8 + u * N * rec:B * 8 + (u + 1) * N * rec]])
    row = 2 * (4 + 2 * s.jdesc.max_frames) if blob == "joint_state" else 2 * 8
    return w[u * N * row:(u + 1) * N * row]


def test_mixed_graph_ids_batch():
    """graph_ids = (1, -1, 0, 2) over a set of two graphs: the biased utterances against the reference, and the two unbiased
    ones (-1, and 2 = G, out of range) against the search built without a context on the same inputs: results, search-state
    records, scorer state and LM state equal bit for bit"""
    r64, biased = _check("mixed")
    assert cases.case("mixed")[5]["ids"] == (1, -1, 0, 2) and len(biased.context) == 2
    plain = _searcher("mixed", ctx=False)
    _search(plain, "mixed")
    _search(biased, "mixed")
    for u in (1, 3):
        for key in ("score", "att", "ctc", "lm", "lm_state", "lm_n", "hyp_tokens", "hyp_len", "finished", "best", "steps"):
            assert torch.equal(_bits(biased.last[key].cpu())[u], _bits(plain.last[key].cpu())[u]), (key, u)
        assert biased.last["bonus"].cpu()[u].abs().max().item() == 0 and biased.last["ctx_state"].cpu()[u].abs().max().item() == 0
        for blob in ("state", "joint_state", "lm_blob"):
            assert torch.equal(_utterance_words(biased, blob, u), _utterance_words(plain, blob, u)), (blob, u)
    assert not torch.equal(_bits(biased.last["score"].cpu())[0], _bits(plain.last["score"].cpu())[0])    # the context is felt where it is on


def test_context_state_follows_the_hypotheses():
    """the parts, tokens and context states after 1, 2, .. k steps (max_steps = 1 .. k) against the float64 history, across a
    step whose kept candidates share a parent while another parent has none: the state must follow the parents, not the slots"""
    dcfg = cases.case("tiny")[0]
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
        print("aed ctx history: %d steps, parents %s, device err %.3e, bound %.3e" % (k, entry["parent"], err, bound))
        assert [h[0] for h in hyps] == [aed_search_ref.strip(t, eos) for t in entry["tokens"]]
        assert [h[2] for h in hyps] == entry["finished"] and err <= bound
        assert [h[-2] for h in hyps] == [_f32(v) for v in entry["bonus"]]
        assert s.last["ctx_state"].cpu()[b].tolist() == entry["ctx_state"]


def test_row_independence():
    """an utterance searched alone and inside a batch of three: the same bits in tokens, scores and context parts"""
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case("tiny")
    batch, alone = _searcher("tiny"), _searcher("tiny", B=1)
    _search(batch, "tiny")
    full = {k: v.cpu() for k, v in batch.last.items()}
    for b in range(3):
        alone.search(memory[b:b + 1].cuda(), mem_len[b:b + 1], ctc_logits=ctc[b:b + 1].cuda(), ctc_log_probs=True)
        for key in ("score", "att", "ctc", "lm", "bonus", "ctx_state", "hyp_tokens", "hyp_len", "finished", "best", "steps"):
            assert torch.equal(_bits(alone.last[key].cpu()), _bits(full[key][b:b + 1])), (key, b)


def _blobs(s):
    return ("state", "ctx_blob") + (("joint_state",) if s.ctc_weight > 0 else ()) + (("lm_blob",) if s.lm is not None else ())


@pytest.mark.parametrize("name", ["w1_p_is_vocab", "beam1"])
def test_frozen_utterances(name):
    """steps issued past an utterance's end are no-ops: polling every step and every 8 steps leave the same bits in the results
    and in ALL state blobs.  The cases are those whose utterances all end before the largest limit, so that poll = 8 does issue
    steps that poll = 1 does not."""
    a, b = _searcher(name, poll=1), _searcher(name, poll=8)
    ra, rb = _search(a, name, detail=True), _search(b, name, detail=True)
    r64 = cases.reference(name)[0]
    print("aed ctx frozen %s: %d steps issued with poll = 1, %d with poll = 8, the utterances took %s" % (
        name, a.steps_issued, b.steps_issued, [r["steps"] for r in r64]))
    assert a.steps_issued == max(r["steps"] for r in r64) < b.steps_issued
    assert ra == rb
    for blob in _blobs(a):
        assert torch.equal(a.last[blob].cpu(), b.last[blob].cpu()), blob
    for key in ("score", "att", "ctc", "bonus", "ctx_state", "hyp_tokens", "finished", "steps"):
        assert torch.equal(_bits(a.last[key].cpu()), _bits(b.last[key].cpu())), key


def test_packed_rows_equal_the_padded_layout():
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case("tiny")
    padded, packed = _searcher("tiny"), _searcher("tiny")
    want = _search(padded, "tiny", detail=True)
    rows = torch.cat([memory[b, :m] for b, m in enumerate(mem_len)]).cuda()
    crow = torch.cat([ctc[b, :m] for b, m in enumerate(mem_len)]).cuda()
    row0 = torch.tensor([0] + list(np.cumsum(mem_len)), dtype=torch.int32)
    got = packed.search_rows(rows, row0, raw_memory=False, ctc_rows=crow, ctc_log_probs=True, detail=True, graph_ids=[0, 0, 0])
    assert got == want
    for key in ("score", "att", "ctc", "lm", "bonus", "ctx_state", "hyp_tokens", "finished", "steps"):
        assert torch.equal(_bits(packed.last[key].cpu()), _bits(padded.last[key].cpu())), key


@pytest.mark.parametrize("name", ["tiny", "att"])
def test_graph_option_gives_the_same_bits(name):
    eager, graph = _searcher(name), _searcher(name, use_graph=True)
    want = _search(eager, name, detail=True)
    for _ in range(2):                                            # the capturing call and a replaying one
        assert _search(graph, name, detail=True) == want
        for blob in _blobs(eager):
            assert torch.equal(graph.last[blob].cpu(), eager.last[blob].cpu()), blob
        for key in ("score", "att", "ctc", "bonus", "ctx_state"):
            assert torch.equal(_bits(graph.last[key].cpu()), _bits(eager.last[key].cpu())), key


def test_without_context_nothing_of_this_exists():
    """context=None: no context blobs, the launches and the bits of the search built without the keyword; and an EMPTY set gives
    every utterance the same bits through the CTX kernels"""
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case("tiny")
    none = _searcher("tiny", ctx=False)
    a = _search(none, "tiny", detail=True)
    assert all(len(h) == 6 for _, hyps in a for h in hyps)
    assert none.cstate is None and none.cscratch is None and none.bdesc is None and none.graph_of is None and none.bias is None
    assert "bonus" not in none.last and "ctx_blob" not in none.last
    from m3asr.aed_search import AttentionBeamSearch
    empty = AttentionBeamSearch(none.rescorer, 3, spec["beam"], max(mem_len), ctc_weight=spec["w"], pre_beam=spec["pre_beam"], lm=none.lm,
                                lm_weight=spec["alpha"], length_bonus=spec["beta"], context=ContextSet([], device="cuda:0", vocab_size=dcfg.vocab))
    b = _search(empty, "tiny", detail=True, graph_ids=None)
    assert [(best, [h[:6] for h in hyps]) for best, hyps in b] == a and all(h[6:] == (0.0, 0.0) for _, hyps in b for h in hyps)
    for blob in ("state", "joint_state", "lm_blob"):
        assert torch.equal(empty.last[blob].cpu(), none.last[blob].cpu()), blob
    zero = _searcher("att", ctx=False, pre_beam=None)
    assert zero.pre_beam == 0 and zero.launches_per_step() == 8 * dcfg.num_blocks + 3


def test_refusals():
    """through Python: a set on another vocabulary, with eos in a phrase, graph_ids of the wrong length or without a context;
    through the C ABI: 16-byte blobs, NULL mismatches, a non-finite weight, an image of another V and one that is none"""
    from m3asr import ops
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, ctc, spec, lm, graphs = cases.case("tiny")
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    good = ContextSet(graphs, device="cuda:0")
    other = ContextSet([ContextGraph([[1, 2]], 12)], device="cuda:0")
    with pytest.raises(_lib.M3Error, match="vocabulary"):
        AttentionBeamSearch(res, 3, 3, 9, context=other)
    with pytest.raises(_lib.M3Error, match="eos"):
        AttentionBeamSearch(res, 3, 3, 9, context=ContextSet([ContextGraph([[1, 10]], 11)], device="cuda:0"))
    with pytest.raises(_lib.M3Error, match="not on"):
        AttentionBeamSearch(res, 3, 3, 9, context=ContextSet(graphs))
    with pytest.raises(_lib.M3Error, match="pre_beam"):
        AttentionBeamSearch(res, 3, 3, 9, context=good, pre_beam=2)      # the pre-beam applies with a context alone
    assert AttentionBeamSearch(res, 3, 3, 9, context=good).pre_beam == 5
    s = AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5, pre_beam=5, context=good)
    mem = memory.cuda()
    with pytest.raises(_lib.M3Error, match="graph_ids"):
        s.search(mem, mem_len, ctc_logits=ctc.cuda(), ctc_log_probs=True, graph_ids=[0, 1])
    assert s.last is None and s.steps_issued == 0
    with pytest.raises(_lib.M3Error, match="without a context"):
        AttentionBeamSearch(res, 3, 3, 9).search(mem, mem_len, graph_ids=[0, 0, 0])
    # the C ABI
    sdesc = ops.aed_search_desc(3, 3, 9, 11, 32, 2, 2, 100)
    d = ops.aed_bias_desc(sdesc, 5)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    cstate, cscr = u8(ops.aed_bias_state_size(d)), u8(ops.aed_bias_scratch_size(d))
    gof = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    rec = ops.aed_bias_record(good.dev, gof, cstate, cscr)
    with pytest.raises(_lib.M3Error, match="V = 12"):
        ops.aed_bias_reset(d, ops.aed_bias_record(other.dev, gof, cstate, cscr))
    broken = good.dev.clone()
    broken[0] = 0
    with pytest.raises(_lib.M3Error, match="header"):
        ops.aed_bias_reset(d, ops.aed_bias_record(broken, gof, cstate, cscr))
    with pytest.raises(_lib.M3Error, match="context state"):
        ops.aed_bias_reset(d, ops.aed_bias_record(good.dev, gof, cstate[:16], cscr))
    with pytest.raises(_lib.M3Error, match="aligned"):
        ops.aed_bias_reset(d, ops.aed_bias_record(good.dev, gof, u8(ops.aed_bias_state_size(d) + 16)[4:], cscr))
    state = u8(ops.aed_search_state_size(sdesc))
    logits = torch.zeros(9, 11, device="cuda:0")
    score = lambda **kw: ops.aed_bias_score(d, state, kw.get("js"), kw.get("scr"), kw.get("ls"), kw.get("lscr"), logits, kw.get("ctc"),   # noqa: E731
                                            kw.get("w", 0.0), kw.get("lm"), kw.get("on"), kw.get("alpha", 0.0), 0.0, True, kw.get("rec", rec))
    with pytest.raises(_lib.M3Error, match="context scratch"):
        score(rec=ops.aed_bias_record(good.dev, gof, cstate, cscr[:16]))
    with pytest.raises(_lib.M3Error, match="null graph_of"):
        score(rec=ops.aed_bias_record(good.dev, None, cstate, cscr))
    with pytest.raises(_lib.M3Error, match="context image"):
        score(rec=ops.aed_bias_record(None, gof, cstate, cscr))
    with pytest.raises(_lib.M3Error, match="exactly when"):
        score(w=0.5)                                                # ctc_weight > 0 without the CTC input and its blobs
    with pytest.raises(_lib.M3Error, match="exactly when"):
        score(js=u8(1024), scr=u8(1024))                            # ... and the blobs without the weight
    with pytest.raises(_lib.M3Error, match="NULL exactly when there is no LM"):
        score(ls=u8(1024), lscr=u8(1024))                           # LM blobs without an LM image
    with pytest.raises(_lib.M3Error, match="not finite"):
        score(alpha=float("nan"))
    with pytest.raises(_lib.M3Error, match="context state"):
        ops.aed_bias_prune(d, state, None, None, None, None, ops.aed_bias_record(None, None, cstate[:16], cscr))
    with pytest.raises(_lib.M3Error, match="together"):
        ops.aed_bias_prune(d, state, u8(1024), None, None, None, rec)
    with pytest.raises(_lib.M3Error, match="context state"):
        ops.aed_bias_result(d, state, ops.aed_bias_record(None, None, cstate[:16], None))
    with pytest.raises(_lib.M3Error, match="state"):
        ops.aed_bias_result(d, state[:16], rec)


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_end_to_end_builder_and_infer(tmp_path):
    """synthetic CTC/attention checkpoint -> builder.py -> infer.py --attention --ctc-weight 0.3 --hotwords words.txt prints what
    CtcDecoder.attention(ctc_weight=0.3, context=) returns, the bonus included, and still runs the separate biased prefix beam
    search; and that is what aed_ctx_ref finds on Engine.hidden() and the forward's own logits with the same phrase list"""
    from m3asr.decode import CtcDecoder
    from m3asr.engine import Engine
    from m3asr.plan import decoder_config_of, load_plan
    from m3asr.rescore import AttentionRescorer
    d = str(tmp_path)
    beam, steps, w, score = 3, 6, 0.3, 2.0
    _run(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--decoder-blocks", "2", "--seed", "4"])
    model = os.path.join(d, "model.pt")
    sd = torch.load(model, map_location="cpu", weights_only=True)
    plan = os.path.join(d, "aed.plan")
    _run(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", model, "-o", plan, "--opt-shape", "2x80"])
    cfg, packed, extra = load_plan(plan)
    dcfg = decoder_config_of(extra)
    phrases = cases.random_phrases(dcfg.vocab, 8, 3)
    words = os.path.join(d, "words.txt")
    with open(words, "w", encoding="utf-8") as f:
        f.write("# hotwords\n" + "".join(" ".join(str(t) for t in p) + "\n" for p in phrases))
    g = torch.Generator().manual_seed(7)
    feat = torch.rand(2, 90, 40, generator=g)
    np.save(os.path.join(d, "feat.npy"), feat.numpy())
    printed = _run(["infer.py", "-p", plan, "-i", os.path.join(d, "feat.npy"), "--attention", "--beam", str(beam), "--max-steps", str(steps),
                    "--ctc-weight", str(w), "--hotwords", words, "--hotword-score", str(score)])
    shown = {int(m.group(1)): (float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)), [int(t) for t in m.group(6).split()])
             for m in re.finditer(r"^utt (\d+) attention: score=(\S+) att=(\S+) ctc=(\S+) bonus=(\S+) finished=\d tokens=([\d ]*)$", printed, re.M)}
    assert sorted(shown) == [0, 1], printed[-2000:]
    assert len(re.findall(r"^utt \d+ biased: ", printed, re.M)) == 2, printed[-2000:]      # the separate CTC search still runs

    graph = ContextGraph([list(p) for p in phrases], dcfg.vocab, score=score)
    ctx = ContextSet([graph], device="cuda:0")
    eng = Engine(cfg, packed, device="cuda:0")
    dec = CtcDecoder(eng, rescorer=AttentionRescorer(packed, dcfg, "cuda:0"))
    lens = torch.full((2,), feat.shape[1], dtype=torch.int32)
    kw = dict(max_steps=steps, ctc_weight=w, context=ctx)
    detail = dec.attention(feat, lens, beam, detail=True, **kw)
    assert [u[0] for u in detail] == [shown[0][4], shown[1][4]] == dec.attention(feat, lens, beam, **kw)
    for b, (best, hyps) in enumerate(detail):
        chosen = next(h for h in hyps if list(h[0]) == best)
        assert ["%.4f" % v for v in (chosen[1], chosen[3], chosen[4], chosen[5])] == ["%.4f" % v for v in shown[b][:4]]
    hidden = eng.hidden().cpu()
    out_lens = eng.buffer("lens", torch.int32)[:2].cpu().tolist()
    logits = dec.forward(feat, lens)["out_nosm"].cpu()
    ctc = torch.log_softmax(logits.double(), dim=-1)
    w32 = float(np.float32(w))                                   # the C ABI takes the weight as a float
    P = min(max(beam, -(-3 * beam // 2)), 64, dcfg.vocab)
    r64 = ref.search(sd, dcfg, hidden, out_lens, ctc, beam, P, w32, None, 0.0, 0.0, [graph], None, True, None, steps, dtype=torch.float64)
    e32 = ref.e32_of(r64, ref.recomputed_parts(sd, dcfg, hidden, out_lens, ctc.float(), r64, w32, None, 0.0, 0.0, [graph], dtype=torch.float32))
    _compare("end to end", detail, r64, e32, max(8 * e32, 1e-5), False)
