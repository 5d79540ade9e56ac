"""LM sets in the attention decoder's beam search (the <CTC, LM[, CTX]> forms of csrc/aed_joint.hip with a set image,
m3_aed_ngram_reset_set; AttentionBeamSearch(lm=NgramLmSet)).

The tiny decoder over V = 16, B = 3, beam 3, pre_beam 5, at most 6 steps, ctc_weight 0 and 0.3, with and without a context,
lm_on = [2, 0, 3] over the members of tests/lm_set_cases.py.  The oracle is the search that exists without sets: an utterance
that picks member j must get the BITS of the single-LM search with lms[j] and lm_weight = ALPHA * float32(scale_j) -- its
detail=True hypotheses and every per-utterance tensor of search.last; the utterance that is off those of a search whose LM is
switched off (its carried lm_state is then 0, no member's start).  The single-LM references are required to differ from each
other on every utterance, so a kernel that walks the wrong member cannot pass.  (tests/aed_lm_ref.py restates the contract
these references implement; tests/test_aed_lm_gpu.py holds them to it.)"""
import functools

import pytest
import torch

import aed_lm_ref  # noqa: F401  (the contract of the single-LM search, the oracle here)
import lm_set_cases as cases
from m3asr.config import DecoderConfig
from m3asr.plan import pack_decoder
from m3asr.weights import make_decoder_weights

pytestmark = pytest.mark.gpu

B, BEAM, PRE_BEAM, STEPS = 3, 3, 5, 6
MEM = (6, 9, 4)
LM_ON = (2, 0, 3)
GRAPHS = (0, -1, 1)
BLOBS = ("state", "joint_state", "lm_blob", "ctx_blob", "done")


@functools.lru_cache(maxsize=None)
def _model():
    """(dcfg, rescorer, memory (B, T, D), ctc log-probabilities (B, T, V)): drawn as tests/aed_lm_cases.py draws them"""
    from m3asr.rescore import AttentionRescorer
    dcfg = DecoderConfig.tiny(vocab=cases.V)
    g = torch.Generator().manual_seed(3)
    sd = make_decoder_weights(dcfg, seed=3)
    sd["after_norm.weight"] = torch.rand(dcfg.dim, generator=g) + 0.5
    sd["after_norm.bias"] = torch.randn(dcfg.dim, generator=g) * 0.1
    sd["decoder.output_layer.bias"] = sd["decoder.output_layer.bias"].clone()
    sd["decoder.output_layer.bias"][dcfg.vocab - 1] += 0.6
    memory = torch.randn(B, max(MEM), dcfg.dim, generator=g)
    ctc = torch.log_softmax(torch.randn(B, max(MEM), dcfg.vocab, generator=g) * 2.0, dim=-1).float()
    return dcfg, AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0"), memory.cuda(), ctc.cuda()


@functools.lru_cache(maxsize=None)
def _members():
    return tuple(m.to("cuda:0") for m in cases.members())


@functools.lru_cache(maxsize=None)
def _set():
    return cases.lm_set().to("cuda:0")


@functools.lru_cache(maxsize=None)
def _context():
    from m3asr.context import ContextGraph, ContextSet
    return ContextSet([ContextGraph(p, cases.V, score=2.0) for p in ([[3, 4], [7]], [[5, 6, 2], [9, 1]])], device="cuda:0")


def _run(lm, lm_weight, lm_on, w, ctx, rows=False):
    """one search -> (detail=True output, {name: per-utterance CPU tensor of search.last})"""
    from m3asr.aed_search import AttentionBeamSearch
    dcfg, res, memory, ctc = _model()
    s = AttentionBeamSearch(res, B, BEAM, STEPS, ctc_weight=w, pre_beam=PRE_BEAM, lm=lm, lm_weight=lm_weight, length_bonus=cases.BETA,
                            context=_context() if ctx else None)
    kw = dict(detail=True, lm_on=lm_on, raw_memory=False)
    if ctx:
        kw["graph_ids"] = list(GRAPHS)
    if rows:
        packed = torch.cat([memory[b, :n] for b, n in enumerate(MEM)])
        row0 = torch.tensor([0, MEM[0], MEM[0] + MEM[1], sum(MEM)], dtype=torch.int32)
        if w > 0:
            kw.update(ctc_rows=torch.cat([ctc[b, :n] for b, n in enumerate(MEM)]), ctc_log_probs=True)
        out = s.search_rows(packed.contiguous(), row0, **kw)
    else:
        if w > 0:
            kw.update(ctc_logits=ctc, ctc_log_probs=True)
        out = s.search(memory, torch.tensor(MEM, dtype=torch.int32), **kw)
    last = {k: v.cpu().clone() for k, v in s.last.items() if k not in BLOBS and v.shape[:1] == (B,)}
    return out, last


@functools.lru_cache(maxsize=None)
def _single(j, w, ctx):
    """the oracle: all three utterances with member j alone and its scaled weight; j = None: member 0 switched off"""
    if j is None:
        return _run(_members()[0], cases.weight(0), [0] * B, w, ctx)
    return _run(_members()[j], cases.weight(j), None, w, ctx)


def _check(got, lm_on, w, ctx, what):
    out, last = got
    for b, on in enumerate(lm_on):
        j = on - 1 if 1 <= on <= 3 else None
        want_out, want_last = _single(j, w, ctx)
        assert out[b] == want_out[b], "%s utterance %d: the hypotheses differ" % (what, b)
        assert set(last) == set(want_last) and {"lm", "lm_state", "lm_n", "score", "hyp_tokens"} <= set(last)
        for k in last:
            if j is None and k == "lm_state":                     # no member's start state is carried along
                assert not last[k][b].any()
                continue
            assert torch.equal(last[k][b], want_last[k][b]), "%s utterance %d: last[%r] differs" % (what, b, k)
        if j is None:
            assert not last["lm"][b].any()


@pytest.mark.parametrize("ctx", [False, True])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_mixed_batch_equals_the_single_lm_searches(w, ctx):
    # the references disagree between the members on every utterance
    for b in range(B):
        lms = [_single(j, w, ctx)[1]["lm"][b] for j in range(3)]
        assert not torch.equal(lms[0], lms[1]) and not torch.equal(lms[1], lms[2]) and not torch.equal(lms[0], lms[2])
    _check(_run(_set(), cases.ALPHA, list(LM_ON), w, ctx), LM_ON, w, ctx, "search")
    _check(_run(_set(), cases.ALPHA, list(LM_ON), w, ctx, rows=True), LM_ON, w, ctx, "search_rows")
    if ctx:
        assert _single(0, w, ctx)[1]["bonus"].abs().max() > 0, "the case does not exercise the bonus"


def test_other_choices_and_refusals():
    """every member in every position, bools, the default (member 0), and an id above the set"""
    for lm_on in ([1, 2, 3], [3, 1, 2], [True, False, 3]):
        _check(_run(_set(), cases.ALPHA, lm_on, 0.3, False), [int(v) for v in lm_on], 0.3, False, "lm_on %r" % (lm_on,))
    _check(_run(_set(), cases.ALPHA, None, 0.0, False), [1, 1, 1], 0.0, False, "default")
    from m3asr import _lib
    with pytest.raises(_lib.M3Error, match="above 3"):
        _run(_set(), cases.ALPHA, [1, 4, 0], 0.0, False)
    with pytest.raises(_lib.M3Error, match="whole number"):
        _run(_set(), cases.ALPHA, [1, 1.5, 0], 0.0, False)


def test_the_old_reset_refuses_a_set_and_the_new_one_takes_a_single_image():
    from m3asr import _lib, ops
    from m3asr.aed_search import AttentionBeamSearch
    dcfg, res, memory, ctc = _model()
    s = AttentionBeamSearch(res, B, BEAM, STEPS, pre_beam=PRE_BEAM, lm=_set(), lm_weight=cases.ALPHA)
    with pytest.raises(_lib.M3Error, match="header"):
        ops.aed_lm_reset(s.ldesc, s.lstate, _set().dev)
    on = torch.tensor([1, 0, 5], dtype=torch.int32).cuda()
    ops.aed_lm_reset_set(s.ldesc, s.lstate, _members()[2].dev, on)
    rows = s.lstate.view(torch.int32)[:B * BEAM * 16].view(B * BEAM, 2, 8)[:, 0, 0].cpu().view(B, BEAM)
    start = _members()[2].start
    assert start != 0 and rows.tolist() == [[start] * BEAM, [0] * BEAM, [start] * BEAM]
    ops.aed_lm_reset_set(s.ldesc, s.lstate, _set().dev, torch.tensor([3, 2, 4], dtype=torch.int32).cuda())
    rows = s.lstate.view(torch.int32)[:B * BEAM * 16].view(B * BEAM, 2, 8)[:, 0, 0].cpu().view(B, BEAM)
    assert rows.tolist() == [[start] * BEAM, [_members()[1].start] * BEAM, [0] * BEAM]
