"""LM sets in the device CTC prefix beam search (m3_ctc_beam_lm_* with a set image, csrc/ctc_beam.hip; CtcBeamSearch(lm=NgramLmSet)).

The oracle is the search that exists without sets: an utterance that picks member j must get the BITS (torch.equal on tokens,
lengths, score, bonus and hyp_lm) of the single-LM search with lms[j] and lm_weight = ALPHA * float32(scale_j), formed in double;
an utterance that is off those of the search without an LM.  That the three members cannot be confused on these inputs is
asserted on the CPU by tests/test_lm_set_host.py (selectivity); here the single-LM references are additionally required to differ
from each other on every utterance.  References are computed once per process and never modified."""
import functools

import pytest
import torch

import lm_set_cases as cases

pytestmark = pytest.mark.gpu

B, T, BEAM = cases.B, cases.T, cases.BEAM
PATTERN = 0x7FA5A5A5                                              # tests/guarded.py's 4-byte guard pattern
GUARD = 4096


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def _topk(t0=0):
    from m3asr import ops
    lp, ix = ops.ctc_topk(cases.ctc_logits()[:, t0:].cuda().contiguous(), BEAM)
    return lp, ix


@functools.lru_cache(maxsize=None)
def _members():
    return tuple(m.to("cuda") for m in cases.members())


@functools.lru_cache(maxsize=None)
def _set():
    return cases.lm_set().to("cuda")


def _path(x):
    ids = x.argmax(-1).tolist()
    return [t for i, t in enumerate(ids) if t != cases.BLANK and (i == 0 or t != ids[i - 1])]


@functools.lru_cache(maxsize=None)
def _context():
    from m3asr.context import ContextGraph, ContextSet
    x = cases.ctc_logits()
    p0, p1 = _path(x[0]), _path(x[2])
    return ContextSet([ContextGraph(p, cases.V, score=1.5, blank=cases.BLANK) for p in ([p0[1:3], p0[4:5]], [p1[0:2], p1[3:5]])],
                      device="cuda")


GRAPHS = (0, 1, -1, 0)


def _search(lm_image, lm_on, alpha, ctx=False, t0=0, chunk=None, restart=None):
    """ops-level fused search of all B utterances over the frames from t0 on, `chunk` frames per advance (default: one advance).
    restart = (frame, slot, lm_on value): after that many frames the slot is reset and continues with the new value.
    -> (tokens, lengths, score, bonus, hyp_lm, n_hyps) on the CPU"""
    from m3asr import ops
    lp, ix = _topk(t0)
    n = lp.shape[1]
    desc = ops.ctc_beam_desc(B, BEAM, T, cases.BLANK, BEAM)
    state = torch.empty(ops.ctc_beam_lm_state_size(desc), dtype=torch.uint8, device="cuda")
    image = _context().dev if ctx else None
    go = _i32(GRAPHS if ctx else [-1] * B)
    on = _i32(lm_on)
    ops.ctc_beam_lm_reset(desc, state)
    c = chunk or n
    for f in range(0, n, c):
        if restart is not None and f == restart[0]:
            ops.ctc_beam_lm_reset(desc, state, _i32([restart[1]]))
            on[restart[1]] = restart[2]
        m = min(c, n - f)
        ops.ctc_beam_lm_advance(desc, state, image, go, lm_image, on, alpha, cases.BETA, lp[:, f:f + m].contiguous(),
                                ix[:, f:f + m].contiguous(), _i32([m] * B))
    out = ops.ctc_beam_lm_nbest(desc, state, image, go, lm_image, on, alpha, cases.BETA, True)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


@functools.lru_cache(maxsize=None)
def _single(j, ctx=False, t0=0):
    """the oracle: every utterance searched with member j alone and its scaled weight (j = None: without an LM)"""
    if j is None:
        return _search(None, [0] * B, cases.ALPHA, ctx, t0)
    return _search(_members()[j].dev, [1] * B, cases.weight(j), ctx, t0)


def _same_row(got, b, want, wb=None, what=""):
    wb = b if wb is None else wb
    for i, name in enumerate(("tokens", "lengths", "score", "bonus", "hyp_lm", "n_hyps")):
        assert torch.equal(got[i][b], want[i][wb]), "%s utterance %d: %s differs" % (what, b, name)


def _check(got, lm_on, ctx=False, what=""):
    for b, on in enumerate(lm_on):
        j = on - 1 if 1 <= on <= 3 else None
        _same_row(got, b, _single(j, ctx), what=what)
        if j is None:
            assert not got[4][b].any(), "an utterance without the LM reports an LM score"
        else:
            assert got[4][b].abs().max() > 0


def test_references_differ_between_members():
    """what makes the equalities below mean something: on every utterance the three single-LM searches disagree"""
    for ctx in (False, True):
        for b in range(B):
            lms = [_single(j, ctx)[4][b] for j in range(3)]
            assert not torch.equal(lms[0], lms[1]) and not torch.equal(lms[1], lms[2]) and not torch.equal(lms[0], lms[2])
            if not ctx:                                           # as the host routine shows on the CPU
                assert len({tuple(_single(j)[0][b, 0].tolist()) for j in range(3)}) >= 2


@pytest.mark.parametrize("ctx", [False, True])
def test_offline_mixed_batch(ctx):
    """B = 4, 20 frames, beam 4, lm_on = [3, 0, 1, 2], scales (1.0, 0.5, 2.0)"""
    got = _search(_set().dev, cases.LM_ON, cases.ALPHA, ctx)
    _check(got, cases.LM_ON, ctx, "offline")
    if ctx:
        assert got[3].abs().max() > 0, "the case does not exercise the bonus"


@pytest.mark.parametrize("ctx", [False, True])
def test_values_outside_the_set_mean_off(ctx):
    for lm_on in ([4, -1, 1, 2], [2, 3, 65, -(2 ** 31)]):
        _check(_search(_set().dev, lm_on, cases.ALPHA, ctx), lm_on, ctx, "lm_on %r" % (lm_on,))


@pytest.mark.parametrize("chunk,frame", [(1, 10), (3, 9), (7, 7)])
def test_streaming_chunks_and_a_restart_with_another_member(chunk, frame):
    """the same frames in chunks of 1, 3 and 7; slot 2 (member 0, start state 0) is restarted mid-run with member 2, whose start
    state is the <s> context: from there on it must be the single-LM search of member 2 over the remaining frames"""
    assert _members()[2].start != 0 and _members()[0].start == 0
    got = _search(_set().dev, cases.LM_ON, cases.ALPHA, chunk=chunk)
    _check(got, cases.LM_ON, what="chunks of %d" % chunk)
    got = _search(_set().dev, cases.LM_ON, cases.ALPHA, chunk=chunk, restart=(frame, 2, 3))
    for b in (0, 1, 3):
        _same_row(got, b, _single(cases.LM_ON[b] - 1 if cases.LM_ON[b] else None), what="restart, chunks of %d" % chunk)
    _same_row(got, 2, _single(2, False, frame), what="the restarted slot, chunks of %d" % chunk)
    assert not torch.equal(got[4][2], _single(0, False, frame)[4][2])


def test_single_image_any_nonzero_lm_on_is_on():
    """a plain NgramLm with lm_on 1 and 7: the single-image path, bit for bit what lm_on = 1 gives"""
    for j in range(3):
        got = _search(_members()[j].dev, [1, 7, -3, 0], cases.weight(j))
        for b in (0, 1, 2):
            _same_row(got, b, _single(j), what="single image")
        _same_row(got, 3, _single(None), what="single image, off")


def test_damaged_set_header_runs_with_the_lm_off_inside_its_guards():
    image = _set().image
    buf = torch.full((GUARD + image.size + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    view = buf[GUARD:GUARD + image.size]
    view.copy_(torch.from_numpy(image))
    assert view.data_ptr() % 16 == 0
    _check(_search(view, cases.LM_ON, cases.ALPHA), cases.LM_ON, what="guarded set")
    view[0] = 0x12345678                                          # neither a set nor a single image
    got = _search(view, cases.LM_ON, cases.ALPHA)
    _check(got, [0] * B, what="damaged header")
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + image.size:] == PATTERN).all())
    # a directory entry that points past the set: that utterance alone runs without the LM
    view.copy_(torch.from_numpy(image))
    view[8 + 4 * 2 + 1] += 4
    _check(_search(view, cases.LM_ON, cases.ALPHA), [0, 0, 1, 2], what="damaged entry")
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + image.size:] == PATTERN).all())


def test_ctc_beam_search_class_takes_a_set():
    """CtcBeamSearch(lm=set): reset(lm_on=) takes ints and bools, refuses an id above the set, keeps a member across restarts of
    other slots, and a restarted slot takes its new member"""
    from m3asr.decode import CtcBeamSearch
    x = cases.ctc_logits().cuda()
    lens = torch.full((B,), T, dtype=torch.int32)
    s = CtcBeamSearch(B, BEAM, T, cases.BLANK, "cuda", lm=_set(), lm_weight=cases.ALPHA, length_bonus=cases.BETA)
    s.reset(lm_on=list(cases.LM_ON))
    s.advance(x, lens)
    _check(tuple(t.cpu() for t in s.nbest_tensors(detail=True)), cases.LM_ON, what="class")
    hyps = s.nbest(detail=True)
    assert len(hyps) == B and all(len(h[0]) == 4 for h in hyps)                 # (prefix, score, bonus, lm): unchanged in shape
    with pytest.raises(ValueError, match="above 3"):
        s.reset(lm_on=[4, 0, 0, 0])
    s.reset(lm_on=[True, False, 2, 3])
    assert s.lm_on.tolist() == [1, 0, 2, 3]
    s.reset(slots=[1], lm_on=[3])                                 # the others keep their member
    assert s.lm_on.tolist() == [1, 3, 2, 3]
    s.advance(x, lens)
    _check(tuple(t.cpu() for t in s.nbest_tensors(detail=True)), [1, 3, 2, 3], what="class, second run")
    assert torch.equal(s.lm_weights().cpu().view(-1), torch.tensor([cases.weight(0), cases.weight(2), cases.weight(1), cases.weight(2)],
                                                                   dtype=torch.float32))
    # a plain NgramLm: flags as ever
    p = CtcBeamSearch(B, BEAM, T, cases.BLANK, "cuda", lm=_members()[1], lm_weight=cases.weight(1), length_bonus=cases.BETA)
    p.reset(lm_on=[1, 7, True, 0])
    assert p.lm_on.tolist() == [1, 1, 1, 0] and p.lm_weights() == cases.weight(1)


def test_attention_rescoring_prior_takes_each_utterances_scaled_weight():
    """AttentionRescorer.rescore over a CtcBeamSearch(lm=set): every utterance's (tokens, prior, att, final) are those of the
    rescoring over the single-LM search of its member with the scaled weight -- the prior is the search's own key, so a wrong
    per-utterance weight shows in prior and final"""
    from m3asr.config import DecoderConfig
    from m3asr.decode import CtcBeamSearch
    from m3asr.plan import pack_decoder
    from m3asr.rescore import AttentionRescorer
    from m3asr.weights import make_decoder_weights
    dcfg = DecoderConfig.tiny(vocab=cases.V)
    g = torch.Generator().manual_seed(7)
    sd = make_decoder_weights(dcfg, seed=7)
    sd["after_norm.weight"] = torch.rand(dcfg.dim, generator=g) + 0.5
    sd["after_norm.bias"] = torch.randn(dcfg.dim, generator=g) * 0.1
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    memory = torch.randn(B, T, dcfg.dim, generator=g).cuda()
    x = cases.ctc_logits().cuda()
    lens = torch.full((B,), T, dtype=torch.int32)

    def rescore(lm, weight, lm_on):
        s = CtcBeamSearch(B, BEAM, T, cases.BLANK, "cuda", lm=lm, lm_weight=weight, length_bonus=cases.BETA)
        s.reset(lm_on=lm_on)
        s.advance(x, lens)
        return res.rescore(memory, lens, s, ctc_weight=0.5)

    got = rescore(_set(), cases.ALPHA, list(cases.LM_ON))
    singles = [rescore(_members()[j], cases.weight(j), [1] * B) for j in range(3)]
    off = rescore(_members()[0], cases.weight(0), [0] * B)
    for b, on in enumerate(cases.LM_ON):
        want = off if on == 0 else singles[on - 1]
        assert got[b] == want[b], "utterance %d" % b
        if on:                                                    # the priors differ between the members' weights
            assert all([h[1] for h in got[b][1]] != [h[1] for h in singles[j][b][1]] for j in range(3) if j != on - 1)
