"""Attention decoding with n-gram LM fusion and a length bonus on the device (m3asr.aed_search with lm=, the <CTC, LM>
instantiations of csrc/aed_joint.hip) against tests/aed_lm_ref.py.

Yardstick, that of tests/test_aed_joint_gpu.py: aed_lm_ref in float64 is the truth; e32 is the largest difference between its
key / att / ctc and the same quantities of the SAME kept candidates recomputed in float32 on the CPU; the device must be within
max(8 e32, 1e-5) on all three.  The device's lm must EQUAL the float32 rounding of the reference's double (both are the same double
sums of the same float32 table entries in the same order), its lm_state and token counts must be equal, and the discrete results
identical; every utterance's float64 decision margin exceeds twice the bound (seeds picked on the CPU, tests/aed_lm_cases.py;
asserted, never skipped).  No bound comes from the device's output; every test prints the device error, e32, the bound and the
margin before it asserts (run with -s)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_lm_cases as cases
import aed_lm_ref as ref
import aed_search_ref
import lm_ref
from m3asr import _lib
from m3asr.plan import pack_decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _searcher(name, B=None, lm=True, **kw):
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, ctc, spec, model, _ = cases.case(name)
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    kw.setdefault("ctc_weight", spec["w"])
    kw.setdefault("pre_beam", spec["pre_beam"])
    if lm:
        kw.update(lm=model.to("cuda:0"), lm_weight=spec["alpha"], length_bonus=spec["beta"], lm_eos=spec["use_eos"])
    return AttentionBeamSearch(res, len(mem_len) if B is None else B, spec["beam"], spec["max_steps"] or max(mem_len), **kw)


def _search(s, name, **kw):
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case(name)
    if s.ctc_weight > 0:
        kw.update(ctc_logits=ctc.cuda(), ctc_log_probs=True)
    if s.lm is not None:
        kw.setdefault("lm_on", spec["lm_on"])
    return s.search(memory.cuda(), torch.tensor(mem_len, dtype=torch.int32), **kw)


def _gap(a, b):
    return 0.0 if a == b else abs(a - b)            # -inf against -inf is exact; against anything else the gap is inf


def _err(hyps, want):
    """largest difference over key, att and ctc; hyps: (tokens, key, finished, att, ctc, lm), want: rows of (key, att, ctc)"""
    return max(max(_gap(h[1], w[0]), _gap(h[3], w[1]), _gap(h[4], w[2])) for h, w in zip(hyps, want))


def _f32(v):
    return float(np.float32(v))


def _compare(tag, out, r64, e32, bound):
    """out: search(detail=True)'s result for the utterances of r64"""
    for b, ((best, hyps), want) in enumerate(zip(out, r64)):
        err = _err(hyps, [(w[1], w[2], w[3]) for w in want["nbest"]])
        print("aed lm %s utterance %d: device err %.3e, e32 %.3e, bound %.3e, margin %.3e, steps %d / limit %d" % (
            tag, b, err, e32, bound, want["margin"], want["steps"], want["limit"]))
        assert want["margin"] > 2 * bound, "the seed leaves utterance %d with a near tie" % b
        assert [h[0] for h in hyps] == [w[0] for w in want["nbest"]]
        assert [h[2] for h in hyps] == [w[4] for w in want["nbest"]]
        assert tuple(best) == want["nbest"][want["best"]][0]
        assert [h[5] for h in hyps] == [_f32(w[5]) for w in want["nbest"]]             # exactly
        assert not any(np.isnan(v) for h in hyps for v in (h[1], h[3], h[4])) and err <= bound, (err, bound)


def _check(name):
    r64, e32, bound = cases.reference(name)
    s = _searcher(name)
    out = _search(s, name, detail=True)
    _compare(name, out, r64, e32, bound)
    last = {k: v.cpu() for k, v in s.last.items()}
    assert last["steps"].tolist() == [r["steps"] for r in r64] and last["done"].tolist() == [1] * len(r64)
    assert last["best"].tolist() == [r["best"] for r in r64]
    assert last["lm_state"].tolist() == [r["lm_state"] for r in r64] and last["lm_n"].tolist() == [r["n"] for r in r64]
    assert s.launches_per_step() == 8 * cases.case(name)[0].num_blocks + 4
    assert _search(s, name) == [list(r["nbest"][r["best"]][0]) for r in r64]      # a second call, without detail
    return r64, s


def test_tiny_model():
    """2 blocks, D 32, dk 16, V 11, beam 3, P 5; memories of 5, 9 and 1 frames in one call; a trigram LM, lm_weight 0.5 and a
    length bonus of 4: walks that find their arc at once, that back off one and two levels, and one that ends on unk_logp"""
    r64, _ = _check("tiny")
    assert [r["limit"] for r in r64] == [5, 9, 1]
    assert {0, 1, 2} <= {lv for r in r64 for lv in cases.kept_levels(r)}
    assert any(h[4] for r in r64 for h in r["nbest"]) and any(h[5] != 0.0 for r in r64 for h in r["nbest"])


@pytest.mark.parametrize("name", ["unigram", "bigram", "backoff", "w0", "w1_p_is_vocab", "beam1", "p64", "frames", "no_eos", "beta_only"])
def test_lms_weights_and_shapes(name):
    """a unigram LM (every walk is state 0); a bigram LM (one level above it); a trigram LM whose kept candidates back off two levels and land on unk_logp;
    ctc_weight = 0 with an LM (the <false, true> instantiation: no CTC input, ctc part 0); w = 1 with P = V = 5; beam 1; P = 64 of
    V = 70 (every lane walks); memories of 63 / 64 / 65 frames (the walk in front of the frame chain's tile edges); use_eos off;
    the length bonus alone (alpha = 0)"""
    r64, s = _check(name)
    spec, lm = cases.case(name)[5], cases.case(name)[6]
    levels = [lv for r in r64 for lv in cases.kept_levels(r)]
    if name == "unigram":
        assert lm.n_states == 1 and set(levels) == {0}
    if name == "bigram":
        assert lm.order == 2 and set(levels) == {0, 1}
    if name == "backoff":
        assert max(levels) >= 2 and sum(cases.kept_unknown(r) for r in r64) >= 1
    if name == "w0":
        assert spec["w"] == 0 and s.jstate is None and s.ctc is None and "joint_state" not in s.last
        assert all(h[3] == 0.0 for r in r64 for h in r["nbest"])
        assert s.last["ctc"].abs().max().item() == 0
    if name == "w1_p_is_vocab":
        assert spec["w"] == 1.0 and spec["pre_beam"] == spec["dcfg"].vocab == 5
    if name == "p64":
        assert spec["pre_beam"] == 64 and spec["dcfg"].vocab == 70
    if name == "frames":
        assert list(spec["mem"]) == [63, 64, 65] and [r["limit"] for r in r64] == [6, 6, 6]
    if name == "no_eos":
        assert not spec["use_eos"] and any(h[4] for r in r64 for h in r["nbest"])
    if name == "beta_only":
        assert spec["alpha"] == 0 and spec["beta"] > 0


def test_real_widths_one_block():
    """D 512 / F 2048 / V 1434 / dk 128, one block, beam 4, P 6, memories of 70 and 37 frames, 12 steps, a 3-gram LM of a few
    thousand n-grams"""
    r64, _ = _check("real")
    assert all(r["limit"] == 12 for r in r64) and cases.case("real")[6].n_grams > 2000


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _utterance_words(s, blob, u):
    """the int32 words of utterance u in a state blob of searcher s: its header and both records of its rows, or its rows of the
    scorer state"""
    N, B = s.beam, s.B
    w = s.last[blob].cpu().view(torch.int32)
    if blob == "state":
        rec = 2 * (2 + 2 * (s.max_steps + 1))
        return torch.cat([w[u * 8:(u + 1) * 8], w[B * 8 + u * N * rec:B * 8 + (u + 1) * N * rec]])
    row = 2 * (4 + 2 * s.jdesc.max_frames)
    return w[u * N * row:(u + 1) * N * row]


def test_mixed_lm_on_batch():
    """lm_on = (1, 0, 1): the fused utterances against the reference, and the one that is switched off against the plain joint
    search of the same inputs: results, search-state records and scorer state equal bit for bit"""
    r64, fused = _check("mixed")
    assert cases.case("mixed")[5]["lm_on"] == (1, 0, 1)
    plain = _searcher("mixed", lm=False)
    _search(plain, "mixed")
    _search(fused, "mixed")
    for key in ("score", "att", "ctc", "hyp_tokens", "hyp_len", "finished", "best", "steps"):
        assert torch.equal(_bits(fused.last[key].cpu())[1], _bits(plain.last[key].cpu())[1]), key
        if key == "score":
            assert not torch.equal(_bits(fused.last[key].cpu())[0], _bits(plain.last[key].cpu())[0])          # the LM is felt where it is on
    assert fused.last["lm"].cpu()[1].abs().max().item() == 0
    for blob in ("state", "joint_state"):
        assert torch.equal(_utterance_words(fused, blob, 1), _utterance_words(plain, blob, 1)), blob


def test_zero_weights_give_the_joint_bits():
    """an LM image with alpha = beta = 0: the walk runs and nothing is added: the plain joint search's bits in the results and in
    both of its state blobs, while lm and lm_state are the reference's"""
    _, fused = _check("zero_weights")
    plain = _searcher("zero_weights", lm=False)
    _search(plain, "zero_weights")
    _search(fused, "zero_weights")
    for key in ("score", "att", "ctc", "hyp_tokens", "hyp_len", "finished", "best", "steps"):
        assert torch.equal(_bits(fused.last[key].cpu()), _bits(plain.last[key].cpu())), key
    for blob in ("state", "joint_state"):
        assert torch.equal(fused.last[blob].cpu(), plain.last[blob].cpu()), blob
    assert fused.last["lm"].abs().max().item() > 0


def test_lm_state_follows_the_hypotheses():
    """the parts, tokens and LM states after 1, 2, .. k steps (max_steps = 1 .. k) against the float64 history, across a step
    whose kept candidates share a parent while another parent has none and a later step that extends them: the LM state must
    follow the parents, not the slots"""
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
        print("aed lm history: %d steps, parents %s, device err %.3e, bound %.3e" % (k, entry["parent"], err, bound))
        assert [h[0] for h in hyps] == [aed_search_ref.strip(t, eos) for t in entry["tokens"]]
        assert [h[2] for h in hyps] == entry["finished"] and err <= bound
        assert [h[5] for h in hyps] == [_f32(v) for v in entry["lm"]]
        assert s.last["lm_state"].cpu()[b].tolist() == entry["lm_state"] and s.last["lm_n"].cpu()[b].tolist() == entry["n"]


def test_row_independence():
    """an utterance searched alone and inside a batch of three: the same bits in tokens, scores and LM parts"""
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case("tiny")
    batch, alone = _searcher("tiny"), _searcher("tiny", B=1)
    _search(batch, "tiny")
    full = {k: v.cpu() for k, v in batch.last.items()}
    for b in range(3):
        alone.search(memory[b:b + 1].cuda(), mem_len[b:b + 1], ctc_logits=ctc[b:b + 1].cuda(), ctc_log_probs=True)
        for key in ("score", "att", "ctc", "lm", "lm_state", "lm_n", "hyp_tokens", "hyp_len", "finished", "best", "steps"):
            assert torch.equal(_bits(alone.last[key].cpu()), _bits(full[key][b:b + 1])), (key, b)


@pytest.mark.parametrize("name", ["w1_p_is_vocab", "beam1", "w0"])
def test_frozen_utterances(name):
    """steps issued past an utterance's end are no-ops: polling every step and every 8 steps leave the same bits in the results
    and in ALL state blobs.  The cases are those whose utterances all end before the largest limit, so that poll = 8 does issue
    steps that poll = 1 does not."""
    a, b = _searcher(name, poll=1), _searcher(name, poll=8)
    ra, rb = _search(a, name, detail=True), _search(b, name, detail=True)
    r64 = cases.reference(name)[0]
    print("aed lm frozen %s: %d steps issued with poll = 1, %d with poll = 8, the utterances took %s" % (
        name, a.steps_issued, b.steps_issued, [r["steps"] for r in r64]))
    assert a.steps_issued == max(r["steps"] for r in r64) < b.steps_issued
    assert ra == rb
    for blob in ("state", "lm_blob") + (("joint_state",) if a.ctc_weight > 0 else ()):
        assert torch.equal(a.last[blob].cpu(), b.last[blob].cpu()), blob
    for key in ("score", "att", "ctc", "lm", "lm_state", "lm_n", "hyp_tokens", "finished", "steps"):
        assert torch.equal(_bits(a.last[key].cpu()), _bits(b.last[key].cpu())), key


def test_packed_rows_equal_the_padded_layout():
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case("tiny")
    padded, packed = _searcher("tiny"), _searcher("tiny")
    want = _search(padded, "tiny", detail=True)
    rows = torch.cat([memory[b, :m] for b, m in enumerate(mem_len)]).cuda()
    crow = torch.cat([ctc[b, :m] for b, m in enumerate(mem_len)]).cuda()
    row0 = torch.tensor([0] + list(np.cumsum(mem_len)), dtype=torch.int32)
    got = packed.search_rows(rows, row0, raw_memory=False, ctc_rows=crow, ctc_log_probs=True, detail=True)
    assert got == want
    for key in ("score", "att", "ctc", "lm", "lm_state", "hyp_tokens", "finished", "steps"):
        assert torch.equal(_bits(packed.last[key].cpu()), _bits(padded.last[key].cpu())), key


@pytest.mark.parametrize("name", ["tiny", "w0"])
def test_graph_option_gives_the_same_bits(name):
    eager, graph = _searcher(name), _searcher(name, use_graph=True)
    want = _search(eager, name, detail=True)
    for _ in range(2):                                            # the capturing call and a replaying one
        assert _search(graph, name, detail=True) == want
        for blob in ("state", "lm_blob") + (("joint_state",) if eager.ctc_weight > 0 else ()):
            assert torch.equal(graph.last[blob].cpu(), eager.last[blob].cpu()), blob
        for key in ("score", "att", "ctc", "lm", "lm_state"):
            assert torch.equal(_bits(graph.last[key].cpu()), _bits(eager.last[key].cpu())), key


def test_without_lm_nothing_of_this_exists():
    """lm=None: no LM blobs, the launches and the bits of the search built without the keywords"""
    from m3asr.aed_search import AttentionBeamSearch
    dcfg, sd, memory, mem_len, ctc, spec, _, _ = cases.case("tiny")
    none = _searcher("tiny", lm=False, lm_weight=0.5, length_bonus=1.0)
    plain = AttentionBeamSearch(none.rescorer, len(mem_len), spec["beam"], max(mem_len), ctc_weight=spec["w"], pre_beam=spec["pre_beam"])
    a, b = _search(none, "tiny", detail=True), _search(plain, "tiny", detail=True)
    assert a == b and all(len(h) == 5 for _, hyps in a for h in hyps)
    assert none.lstate is None and none.lscratch is None and none.ldesc is None and none.lm_on is None
    assert "lm" not in none.last and "lm_blob" not in none.last
    assert torch.equal(none.last["state"].cpu(), plain.last["state"].cpu())
    zero = _searcher("tiny", lm=False, ctc_weight=0.0, pre_beam=None)
    assert zero.pre_beam == 0 and zero.launches_per_step() == 8 * dcfg.num_blocks + 3


def test_refusals():
    """an LM of another vocabulary, a NaN lm_weight or length_bonus, an LM that was not moved to the device, lm_on of the wrong
    length or without an LM: M3Error before any launch; and the C ABI's own refusals of an image of another V, an image that is
    none, and non-finite weights"""
    from m3asr import ops
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.lm import NgramLm
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len, ctc, spec, lm, _ = cases.case("tiny")
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    other = NgramLm(cases.lm_grams(12, 2, 5, 10, 1)[1], 12).to("cuda:0")
    with pytest.raises(_lib.M3Error, match="vocabulary"):
        AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5, lm=other)
    lm.to("cuda:0")
    for kw in (dict(lm_weight=float("nan")), dict(length_bonus=float("nan")), dict(lm_weight=float("inf"))):
        with pytest.raises(_lib.M3Error, match="not finite"):
            AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5, lm=lm, **kw)
    host = NgramLm(cases.lm_grams(11, 2, 5, 10, 1)[1], 11)
    with pytest.raises(_lib.M3Error, match="not on"):
        AttentionBeamSearch(res, 3, 3, 9, lm=host)
    with pytest.raises(_lib.M3Error, match="pre_beam"):
        AttentionBeamSearch(res, 3, 3, 9, lm=lm, pre_beam=2)          # the pre-beam applies with an LM alone
    assert AttentionBeamSearch(res, 3, 3, 9, lm=lm).pre_beam == 5
    s = AttentionBeamSearch(res, 3, 3, 9, ctc_weight=0.5, pre_beam=5, lm=lm, lm_weight=0.5)
    mem = memory.cuda()
    with pytest.raises(_lib.M3Error, match="lm_on"):
        s.search(mem, mem_len, ctc_logits=ctc.cuda(), ctc_log_probs=True, lm_on=[1, 0])
    assert s.last is None and s.steps_issued == 0
    z = AttentionBeamSearch(res, 3, 3, 9)
    with pytest.raises(_lib.M3Error, match="without an LM"):
        z.search(mem, mem_len, lm_on=[1, 1, 1])
    w0 = AttentionBeamSearch(res, 3, 3, 9, lm=lm, lm_weight=0.5)
    with pytest.raises(_lib.M3Error, match="ctc_weight = 0"):
        w0.search(mem, mem_len, ctc_logits=ctc.cuda())
    # the C ABI
    sdesc = ops.aed_search_desc(3, 3, 9, 11, 32, 2, 2, 100)
    for p in (2, 65, 12):
        with pytest.raises(_lib.M3Error, match="pre_beam"):
            ops.aed_lm_desc(sdesc, p)
    d = ops.aed_lm_desc(sdesc, 5)
    lstate = torch.zeros(ops.aed_lm_state_size(d), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_lib.M3Error, match="V = 12"):
        ops.aed_lm_reset(d, lstate, other.dev)
    broken = lm.dev.clone()
    broken[0] = 0
    with pytest.raises(_lib.M3Error, match="header"):
        ops.aed_lm_reset(d, lstate, broken)
    with pytest.raises(_lib.M3Error, match="LM state"):
        ops.aed_lm_reset(d, lstate[:16], lm.dev)
    lscr = torch.zeros(ops.aed_lm_scratch_size(d), dtype=torch.uint8, device="cuda:0")
    state = torch.zeros(ops.aed_search_state_size(sdesc), dtype=torch.uint8, device="cuda:0")
    logits, on = torch.zeros(9, 11, device="cuda:0"), torch.ones(3, dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.M3Error, match="not finite"):
        ops.aed_lm_score(d, state, None, None, lstate, lscr, logits, None, 0.0, lm.dev, on, float("nan"), 0.0)
    with pytest.raises(_lib.M3Error, match="exactly when"):
        ops.aed_lm_score(d, state, None, None, lstate, lscr, logits, None, 0.5, lm.dev, on, 0.5, 0.0)
    with pytest.raises(_lib.M3Error, match="LM scratch"):
        ops.aed_lm_score(d, state, None, None, lstate, lscr[:16], logits, None, 0.0, lm.dev, on, 0.5, 0.0)


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_end_to_end_builder_and_infer(tmp_path):
    """synthetic CTC/attention checkpoint -> builder.py -> infer.py --attention --ctc-weight 0.3 --lm lm.arpa prints what
    CtcDecoder.attention(ctc_weight=0.3, lm=) returns, all three parts included; and that is what aed_lm_ref finds on
    Engine.hidden() and the forward's own logits with the LM compiled from the same ARPA text"""
    from m3asr.decode import CtcDecoder
    from m3asr.engine import Engine
    from m3asr.lm import NgramLm
    from m3asr.plan import decoder_config_of, load_plan
    from m3asr.rescore import AttentionRescorer
    d = str(tmp_path)
    beam, steps, w, alpha, beta = 3, 6, 0.3, 0.5, 0.25
    _run(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--decoder-blocks", "2", "--seed", "4"])
    model = os.path.join(d, "model.pt")
    sd = torch.load(model, map_location="cpu", weights_only=True)
    plan = os.path.join(d, "aed.plan")
    _run(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", model, "-o", plan, "--opt-shape", "2x80"])
    cfg, packed, extra = load_plan(plan)
    dcfg = decoder_config_of(extra)
    _, text = lm_ref.random_arpa(np.random.default_rng(5), dcfg.vocab, 3, min(12, dcfg.vocab - 1), 40)
    arpa = os.path.join(d, "lm.arpa")
    with open(arpa, "w", encoding="utf-8") as f:
        f.write(text)
    g = torch.Generator().manual_seed(7)
    feat = torch.rand(2, 90, 40, generator=g)
    np.save(os.path.join(d, "feat.npy"), feat.numpy())
    printed = _run(["infer.py", "-p", plan, "-i", os.path.join(d, "feat.npy"), "--attention", "--beam", str(beam), "--max-steps", str(steps),
                    "--ctc-weight", str(w), "--lm", arpa, "--lm-weight", str(alpha), "--length-bonus", str(beta)])
    shown = {int(m.group(1)): (float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)), [int(t) for t in m.group(6).split()])
             for m in re.finditer(r"^utt (\d+) attention: score=(\S+) att=(\S+) ctc=(\S+) lm=(\S+) finished=\d tokens=([\d ]*)$", printed, re.M)}
    assert sorted(shown) == [0, 1], printed[-2000:]
    assert "fused:" not in printed                                 # the LM went into the attention search, not a prefix beam search

    lm = NgramLm.from_arpa(text, None, vocab_size=dcfg.vocab).to("cuda:0")
    eng = Engine(cfg, packed, device="cuda:0")
    dec = CtcDecoder(eng, rescorer=AttentionRescorer(packed, dcfg, "cuda:0"))
    lens = torch.full((2,), feat.shape[1], dtype=torch.int32)
    kw = dict(max_steps=steps, ctc_weight=w, lm=lm, lm_weight=alpha, length_bonus=beta)
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
    r64 = ref.search(sd, dcfg, hidden, out_lens, ctc, beam, P, w32, lm, alpha, beta, True, None, steps, dtype=torch.float64)
    e32 = ref.e32_of(r64, ref.recomputed_parts(sd, dcfg, hidden, out_lens, ctc.float(), r64, w32, alpha, beta, dtype=torch.float32))
    _compare("end to end", detail, r64, e32, max(8 * e32, 1e-5))
