"""CPU tier of CTC blank-frame skipping (include/m3asr.h "m3_wfst_skip"): the host restatement
(tests/wfst_skip_ref.py) on cases where the re-insert rule decides the answer, its invariance under the way an utterance is
cut into chunks, the library's refusals (host-only: every one is taken before a launch), and StreamPool(words=True) over a
stand-in decoder.  The device tier (tests/test_wfst_skip_gpu.py) holds the kernel to this restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import wfst_cases as WC
import wfst_ref as R
import wfst_skip_ref as S
from m3asr import _lib, ops
from m3asr._lib import M3Error, WfstSkipDesc
from m3asr.serve import StreamPool, WordSegment
from m3asr.wfst import DecodingGraph

P = 0.98
TOY_ALIGNMENTS = ([3, 0, 3], [0, 3, 3, 0, 0, 3, 0], [1, 2, 0, 0, 3, 0, 3, 0, 2, 1], [1, 0, 2, 0, 0, 1, 1, 2, 2, 3, 0])
THRESHOLDS = (0.5, 0.7)


def _log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def _toy(ali, reinsert=True):
    """-> (kept real frames, words with the graph's final weights) of the skipped search on the alignment's peaked logits"""
    g = DecodingGraph.from_lexicon(WC.TOY_LEXICON, 5)
    logp = _log_softmax(WC.peaked_logits(ali, 5, 8.0))
    s = S.RefSkipSearch(g, 8.0, 50, P, reinsert=reinsert).advance(logp)
    return s.state.map, s.result(True)["words"], R.RefSearch(g, 8.0, 50).advance(logp).result(True)["words"]


def test_reinsertion_keeps_two_equal_tokens_apart():
    kept, words, plain = _toy([3, 0, 3])
    assert kept == [0, 1, 2] and words == [3] == plain
    kept, words, _ = _toy([3, 0, 3], reinsert=False)
    assert kept == [0, 2] and words == []                     # the two 3s merged: no word is spelled 3
    kept, words, plain = _toy([1, 2, 0, 0, 3, 0, 3, 0, 2, 1])
    assert words == [1, 3, 4] == plain and kept == [0, 1, 4, 5, 6, 8, 9]
    assert _toy([1, 2, 0, 0, 3, 0, 3, 0, 2, 1], reinsert=False)[1] == [2, 4]


@pytest.mark.parametrize("ali", TOY_ALIGNMENTS)
def test_peaked_alignments_give_the_unskipped_words(ali):
    """Only for these peaked cases: skipping is an approximation, and nothing else compares skipped to unskipped."""
    kept, words, plain = _toy(ali)
    assert words == plain and len(words) > 0 and len(kept) <= len(ali)


def _cut(logp, blank, thr, chunk):
    st = S.SkipState(blank)
    rows = [S.select(logp[t0:t0 + chunk], blank, thr, st) for t0 in range(0, len(logp), chunk)]
    assert all(len(r) <= min(chunk, len(logp) - t0) + 1 for r, t0 in zip(rows, range(0, len(logp), chunk)))
    return np.concatenate(rows) if rows else np.zeros((0, logp.shape[1]), np.float32), st


@pytest.mark.parametrize("p", THRESHOLDS)
def test_the_selection_does_not_depend_on_the_cut(p):
    thr = S.log_thresh(p)
    seen = kept = reins = 0
    for seed in WC.RANDOM_SEEDS:
        logp = WC.random_case(seed)["logp"]
        whole_state = S.SkipState(0)
        whole = S.select(logp, 0, thr, whole_state)
        assert whole_state.n_seen == len(logp) and whole_state.n_kept == len(whole) == len(whole_state.map) > 0
        assert whole_state.map == sorted(whole_state.map) and all(0 <= f < len(logp) for f in whole_state.map)
        for f, row in zip(whole_state.map, whole):
            assert np.array_equal(row.view(np.int32), logp[f].view(np.int32))
        for chunk in (1, 7):
            rows, st = _cut(logp, 0, thr, chunk)
            assert np.array_equal(rows.view(np.int32), whole.view(np.int32)) and st.map == whole_state.map
            assert (st.n_seen, st.n_kept, st.last_blank, st.last_best, st.reinserted) == (
                whole_state.n_seen, whole_state.n_kept, whole_state.last_blank, whole_state.last_best, whole_state.reinserted)
        seen, kept, reins = seen + len(logp), kept + len(whole), reins + whole_state.reinserted
    assert seen == 1192 and reins >= 10                          # the rule is known to fire
    assert (kept, reins) == {0.5: (766, 61), 0.7: (1037, 21)}[p]


def test_map_frames_of_the_restatement():
    st = S.SkipState(0)
    assert S.map_frames([0], st) == [0]                         # nothing seen: the frame of a word made at reset
    S.select(np.array([[0.0, -9.0]] * 3, np.float32), 0, S.log_thresh(0.5), st)
    assert st.n_kept == 0 and S.map_frames([0], st) == [3]      # seen but none decoded: the frames seen, not 0
    S.select(np.array([[-9.0, 0.0]] * 2, np.float32), 0, S.log_thresh(0.5), st)
    assert st.map == [3, 4] and S.map_frames([0, 1, 2], st) == [3, 4, 5] and S.map_frames([0, 1], st, max_frames=1) == [3, 5]


def _desc(B=2, V=5, blank=0, max_frames=8, thresh=-0.5):
    return WfstSkipDesc(B, V, blank, max_frames, thresh)


@pytest.mark.parametrize("kw,word", [(dict(V=0), "V ="), (dict(blank=-1), "blank"), (dict(blank=5), "blank"), (dict(max_frames=-1), "max_frames"),
                                     (dict(thresh=float("nan")), "NaN"), (dict(B=-1), "B =")])
def test_bad_descriptors_are_refused(kw, word):
    lib = _lib.load()
    assert lib.m3_wfst_skip_state_size(C.byref(_desc(**kw))) == 0 and word in _lib.last_error()
    if "B" not in kw:
        with pytest.raises(M3Error, match=word):
            ops.wfst_skip_desc(2, kw.get("V", 5), kw.get("blank", 0), kw.get("max_frames", 8), kw.get("thresh", -0.5))


def test_calls_refuse_before_any_launch():
    """Host memory stands in for the device's: every refusal is taken before a launch, so nothing is read from it."""
    lib = _lib.load()
    d = _desc()
    need = lib.m3_wfst_skip_state_size(C.byref(d))
    assert need == 2 * 96 and lib.m3_wfst_skip_state_size(C.byref(_desc(B=0))) == 0      # (8 + 5 + 8) words = 84 bytes -> 96
    raw = np.zeros(need + 64, dtype=np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16
    buf = np.zeros(64, dtype=np.int32).ctypes.data
    ok = dict(state=base, bytes=need, logp=buf, ld=5, T=3, nf=buf, out=buf, ld_out=5, nk=buf)

    def select(**kw):
        a = dict(ok, **kw)
        return lib.m3_wfst_skip_select(C.byref(a.get("desc", d)), a["state"], a["bytes"], a["logp"], a["ld"], a["T"], a["nf"], a["out"],
                                       a["ld_out"], a["nk"], None)

    for kw, word in ((dict(bytes=need - 1), "bytes"), (dict(state=base + 4), "aligned"), (dict(state=None), "null"), (dict(ld=4), "ld = 4"),
                     (dict(ld_out=4), "ld_out = 4"), (dict(logp=None), "null pointer"), (dict(nf=None), "null pointer"),
                     (dict(out=None), "null pointer"), (dict(nk=None), "null pointer"), (dict(T=-1), "T_chunk"),
                     (dict(desc=_desc(blank=7)), "blank")):
        assert select(**kw) != 0 and word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.m3_wfst_skip_reset(C.byref(d), base, need - 1, None, 0, None) != 0 and "bytes" in _lib.last_error()
    assert lib.m3_wfst_skip_reset(C.byref(d), base, need, buf, 3, None) != 0 and "slots" in _lib.last_error()
    assert lib.m3_wfst_skip_reset(C.byref(d), base + 8, need, None, 0, None) != 0 and "aligned" in _lib.last_error()
    assert lib.m3_wfst_skip_map_frames(C.byref(d), base, need, None, 4, buf, None) != 0 and "null pointer" in _lib.last_error()
    assert lib.m3_wfst_skip_map_frames(C.byref(d), base, need, buf, -1, buf, None) != 0 and "ld_frames" in _lib.last_error()
    assert lib.m3_wfst_skip_map_frames(C.byref(d), base, need - 1, buf, 4, buf, None) != 0 and "bytes" in _lib.last_error()
    assert lib.m3_wfst_skip_counts(C.byref(d), base, need, buf, None, None) != 0 and "null pointer" in _lib.last_error()
    assert lib.m3_wfst_skip_counts(C.byref(d), None, need, buf, buf, None) != 0 and "null" in _lib.last_error()
    assert lib.m3_wfst_skip_counts(C.byref(_desc(thresh=float("nan"))), base, need, buf, buf, None) != 0 and "NaN" in _lib.last_error()


def test_blank_skip_outside_the_open_interval_is_refused():
    from m3asr.wfst import CtcWfstSearch
    g = DecodingGraph.from_lexicon(WC.TOY_LEXICON, 5)
    g.dev = torch.zeros(1, dtype=torch.int32)                   # the check comes before anything touches the device
    for p in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(M3Error, match="blank_skip"):
            CtcWfstSearch(g, 1, 4, blank_skip=p)


# ---- StreamPool(words=True) over a stand-in decoder
class _Info:
    def __init__(self, rule, frame):
        self.rule, self.frame, self.first_speech, self.last_speech = rule, frame, 1, frame - 1


class _WordsDecoder:
    """What StreamPool(segment=True, words=True) needs of a decoder.  A slot's endpoint fires after `fire_after` chunks; its
    prefix best and its words come from the scripts, one entry per segment of the slot."""

    class _Ep:
        frame_ms = 40

        def length_bound(self):
            return None

    def __init__(self, c, prefixes, words, fire_after=2, graph=True):
        self.c, self.prefixes, self.script, self.fire_after = c, prefixes, words, fire_after
        self.endpoint = self._Ep()
        self.graph = object() if graph else None
        self.chunks, self.segment_no, self.calls = {}, {}, []

    def reset(self, slots=None):
        self.calls.append(("reset", list(slots)))
        for b in slots:
            self.segment_no[b] = self.segment_no.get(b, -1) + 1
            self.chunks[b] = 0

    def step(self, window, valid):
        for b, v in enumerate(valid.tolist()):
            if v:
                self.chunks[b] += 1

    def endpoints(self, slots=None):
        return [_Info(2 if self.chunks[b] >= self.fire_after else 0, self.chunks[b] * self.c - 1) for b in slots]

    def finish(self, slots=None):
        return [[(tuple(self.prefixes[self.segment_no[b] % len(self.prefixes)]), -1.0)] for b in slots]

    def words(self, slots=None, final=False, detail=False):
        self.calls.append(("words", list(slots), final, detail))
        out = []
        for b in slots:
            ws, fs = self.script[self.segment_no[b] % len(self.script)]
            out.append(dict(words=list(ws), frames=list(fs), cost=1.5, reached_final=True, status=0) if detail else list(ws))
        return out


def test_stream_pool_files_word_segments_in_session_time():
    c, idim = 4, 3
    window = 4 * c + 3
    # segment 0: a prefix and words; segment 1: no prefix but a word (filed); segment 2: neither (not filed)
    dec = _WordsDecoder(c, prefixes=[(7, 8), (), ()], words=[([5, 6], [1, 6]), ([9], [2]), ([], [])])
    pool = StreamPool(dec, B=2, chunk=c, input_dim=idim, segment=True, words=True, max_frames=64)
    a, b = pool.open(), pool.open()
    assert pool.words(a) == ([5, 6], [40, 240]) and dec.calls[-1] == ("words", [0], False, True)
    for sid in (a, b):
        pool.push(sid, torch.ones(6 * 4 * c + window, idim))
    assert sorted(pool.step()) == [a, b] and pool.segments(a) == []
    dec.calls.clear()
    assert sorted(pool.step()) == [a, b]                         # both fire: ONE words() call, before either slot is restarted
    assert dec.calls == [("words", [0, 1], True, True), ("reset", [0]), ("reset", [1])]
    seg, = pool.segments(a)
    assert isinstance(seg, WordSegment) and seg.words == [5, 6] and seg.word_ms == [40, 240] and seg.cost == 1.5 and seg.reached_final
    assert seg[:5] == (2, 40, (2 * c - 1) * 40, [((7, 8), -1.0)], 2 * c - 1) and pool.offset_ms(a) == 2 * c * 40
    assert pool.words(a, final=True) == ([9], [(2 * c + 2) * 40])
    pool.step(), pool.step()                                     # the second segment: no prefix, one word -> filed, in session time
    seg, = pool.segments(a)
    assert seg.nbest[0][0] == () and seg.words == [9] and seg.word_ms == [(2 * c + 2) * 40] and seg.end_frame == 4 * c - 1
    pool.step(), pool.step()                                     # the third: neither -> not filed, the offset moves on all the same
    assert pool.segments(a) == [] and pool.offset_ms(a) == 6 * c * 40
    assert len(pool.segments(b)) == 2
    pool.close(a), pool.close(b)


def test_stream_pool_words_refusals():
    c = 4
    with pytest.raises(M3Error, match="graph"):
        StreamPool(_WordsDecoder(c, [()], [([], [])], graph=False), B=1, chunk=c, input_dim=3, words=True)
    dec = _WordsDecoder(c, [()], [([], [])])
    dec.rescorer, dec.rescore, dec.aligner, dec.align = object(), (lambda **kw: None), object(), (lambda **kw: None)
    with pytest.raises(M3Error, match="rescore"):
        StreamPool(dec, B=1, chunk=c, input_dim=3, segment=True, words=True, rescore=True, max_frames=64)
    with pytest.raises(M3Error, match="timestamps"):
        StreamPool(dec, B=1, chunk=c, input_dim=3, segment=True, words=True, timestamps=True, max_frames=64)
    pool = StreamPool(dec, B=1, chunk=c, input_dim=3)            # a pool without words=True: as before, and words() refuses
    sid = pool.open()
    with pytest.raises(M3Error, match="words=True"):
        pool.words(sid)
