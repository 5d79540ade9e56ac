"""CTC forced alignment, the parts that need no GPU: the restatement tests/ctc_align_ref.py against brute force,
its tie rules, the C surface (exports, descriptor validation, the workspace query), the host-side refusals of CtcAligner and
the session-time arithmetic of StreamPool(timestamps=True) over a scripted decoder."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ctc_align_ref as R
from m3asr import _lib, ops
from m3asr.decode import EndpointConfig, EndpointInfo


# ---------------------------------------------------------------- the restatement
def _tiny_cases():
    """every (V, T, y) with V <= 4, T <= 6, L <= 3 over non-blank tokens"""
    for V in (2, 3, 4):
        for T in range(1, 7):
            for L in range(0, 4):
                for y in itertools.product(range(1, V), repeat=L):
                    yield V, T, list(y)


def test_restatement_equals_brute_force():
    """score = the maximum over all V^T labellings that collapse to y; the path collapses to y, is a legal walk, and re-scores
    to the score; infeasible (T, y) are status 1; float32 and float64 agree on the path when the emissions are multiples of 1/4"""
    rng = np.random.default_rng(0)
    feasible = infeasible = with_repeats = 0
    for V, T, y in _tiny_cases():
        e = (-rng.integers(0, 17, size=(T, V)) / 4.0).astype(np.float32)
        want = R.brute_force(e, y)
        r64, r32 = R.ctc_align_ref(e, y, 0, np.float64), R.ctc_align_ref(e, y, 0, np.float32)
        if want == -np.inf:
            infeasible += 1
            assert T < len(y) + R.repeats(y)
            for r in (r64, r32):
                assert r.status == R.NO_ALIGNMENT and r.score == -np.inf and (r.state == -1).all()
                assert (r.start == -1).all() and (r.end == -1).all() and (r.peak == -1).all() and np.isneginf(r.peak_logp).all()
            continue
        feasible += 1
        with_repeats += R.repeats(y) > 0
        assert r64.status == r32.status == R.OK
        assert float(r64.score) == want == float(r32.score), (V, T, y)
        assert np.array_equal(r64.state, r32.state)
        labels = R.path_labels(r64.state, y)
        assert R.collapse(labels) == y and R.is_valid_path(list(r64.state), y)
        assert sum(float(e[t, v]) for t, v in enumerate(labels)) == want
        for i in range(len(y)):
            span = [t for t, s in enumerate(r64.state) if s == 2 * i + 1]
            assert (r64.start[i], r64.end[i]) == (span[0], span[-1] + 1) and span == list(range(span[0], span[-1] + 1))
            col = e[span[0]:span[-1] + 1, y[i]]
            assert r64.peak[i] == span[0] + int(np.argmax(col)) and r64.peak_logp[i] == col.max()
    print("restatement: %d feasible, %d infeasible, %d feasible with a repeated token" % (feasible, infeasible, with_repeats))
    assert feasible > 200 and infeasible > 50 and with_repeats > 50
    empty = R.ctc_align_ref(np.zeros((0, 3), np.float32), [])
    assert empty.status == R.OK and empty.score == 0 and len(empty.state) == 0
    assert R.ctc_align_ref(np.zeros((0, 3), np.float32), [1]).status == R.NO_ALIGNMENT
    for bad in ([0], [3], [-1], [1, 0, 2]):
        assert R.ctc_align_ref(np.zeros((4, 3), np.float32), bad).status == R.BAD_INPUT


def test_tie_rules():
    """all emissions equal: every move ties, stay wins over step over skip, so the walk leaves as LATE as it can and the end
    state is S - 1; a strictly better S - 2 takes the end"""
    r = R.ctc_align_ref(np.zeros((6, 3), np.float32), [1, 2])
    # backtrace from S - 1 = 4 preferring stay: the moves are forced only when the remaining frames run out
    assert r.state.tolist() == [1, 3, 4, 4, 4, 4] and r.score == 0
    assert (r.start.tolist(), r.end.tolist(), r.peak.tolist()) == ([0, 1], [1, 2], [0, 1])
    # a repeated token cannot be skipped into: the blank between the two is visited
    r = R.ctc_align_ref(np.zeros((6, 3), np.float32), [1, 1])
    assert r.state.tolist() == [1, 2, 3, 4, 4, 4]
    # -inf against -inf is a tie too: the unreachable cells record `stay`
    e = np.zeros((3, 2), np.float32)
    r = R.ctc_align_ref(e, [1])
    assert r.state.tolist() == [1, 2, 2]
    # the end: S - 2 only when strictly greater
    e = np.zeros((2, 2), np.float32)
    e[1, 0] = -1.0                                         # ending in the last blank costs 1
    assert R.ctc_align_ref(e, [1]).state.tolist() == [1, 1]
    # the peak is the earliest of equal maxima
    e = np.full((5, 2), -1.0, np.float32)
    e[:, 0] = -9.0
    r = R.ctc_align_ref(e, [1])
    assert (r.start[0], r.end[0], r.peak[0], r.peak_logp[0]) == (0, 5, 0, -1.0)


# ---------------------------------------------------------------- the C surface
NEW = ("m3_ctc_align_workspace_size", "m3_ctc_align_emit", "m3_ctc_align_path")


def test_new_exports_and_unchanged_abi_version():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.m3_abi_version() == 10
    assert [f[0] for f in _lib.CtcAlignDesc._fields_] == ["n", "V", "blank", "max_frames", "max_tokens"]


def _size(n=4, V=1434, blank=0, max_frames=125, max_tokens=40):
    return _lib.load().m3_ctc_align_workspace_size(ctypes.byref(_lib.CtcAlignDesc(n, V, blank, max_frames, max_tokens)))


@pytest.mark.parametrize("kw,word", [(dict(n=-1), "n"), (dict(V=0), "V"), (dict(blank=-1), "blank"), (dict(blank=1434), "blank"),
                                     (dict(max_frames=-1), "max_frames"), (dict(max_tokens=-1), "max_tokens"),
                                     (dict(max_tokens=4001), "max_tokens"), (dict(max_frames=(1 << 20) + 1), "max_frames"),
                                     (dict(max_frames=1 << 20, max_tokens=4000), "overflows"),
                                     (dict(n=1 << 20, max_frames=1 << 12), "overflows")])
def test_workspace_query_refuses_bad_descriptors(kw, word):
    assert _size(**kw) == 0
    assert word in _lib.last_error()
    with pytest.raises(_lib.M3Error):
        ops.ctc_align_desc(**dict(dict(n=4, V=1434, blank=0, max_frames=125, max_tokens=40), **kw))


def test_workspace_query_grows_with_frames_and_tokens():
    assert _lib.load().m3_ctc_align_workspace_size(None) == 0
    assert _size() >= 4 * 125 * 81
    assert _size(n=0) > 0 and _size(max_frames=0) > 0 and _size(max_tokens=0) >= 4 * 125     # never 0 for a descriptor it takes
    by_frames = [_size(max_frames=f) for f in (0, 1, 2, 63, 64, 65, 125, 126, 1300, 5000)]
    by_tokens = [_size(max_tokens=t) for t in (0, 1, 31, 32, 33, 40, 41, 600, 4000)]
    assert by_frames == sorted(by_frames) and by_tokens == sorted(by_tokens)
    assert by_frames[-1] > by_frames[0] and by_tokens[-1] > by_tokens[0]


def test_launchers_refuse_on_the_host():
    """what is refused before a kernel is launched needs no device: a short workspace, ldl < V, null pointers"""
    lib = _lib.load()
    d = _lib.CtcAlignDesc(2, 10, 0, 8, 3)
    one = ctypes.c_void_p(256)                             # never dereferenced: every call below fails its checks first
    assert lib.m3_ctc_align_emit(ctypes.byref(d), one, 9, one, one, one, one, one, None) != 0 and "ldl" in _lib.last_error()
    assert lib.m3_ctc_align_emit(ctypes.byref(d), None, 10, one, one, one, one, one, None) != 0 and "null" in _lib.last_error()
    need = lib.m3_ctc_align_workspace_size(ctypes.byref(d))
    args = [one] * 4
    assert lib.m3_ctc_align_path(ctypes.byref(d), *args, one, need - 1, *([one] * 7), None) != 0 and "workspace" in _lib.last_error()
    assert lib.m3_ctc_align_path(ctypes.byref(d), *args, None, need, *([one] * 7), None) != 0 and "null" in _lib.last_error()
    bad = _lib.CtcAlignDesc(2, 10, 10, 8, 3)
    assert lib.m3_ctc_align_path(ctypes.byref(bad), *args, one, need, *([one] * 7), None) != 0 and "blank" in _lib.last_error()


def test_aligner_refuses_bad_tokens_before_anything_is_launched():
    """the token check runs on the host, in front of every device call: a CPU tensor stands in for the logits"""
    from m3asr.align import Alignment, CtcAligner
    assert Alignment._fields == ("tokens", "start", "end", "peak", "conf", "score", "states", "ok", "start_ms", "end_ms", "peak_ms")
    al = CtcAligner(10, blank=0, device="cpu")
    logits = torch.zeros(2, 5, 10)
    for tokens in ([[1, 0], [2]], [[1], [10]], [[-1], []]):
        with pytest.raises(ValueError, match="token"):
            al.align(logits, [5, 5], tokens)
    with pytest.raises(ValueError, match="lens"):
        al.align(logits, [5, 6], [[1], [2]])
    with pytest.raises(ValueError, match="token lists"):
        al.align_rows(logits.reshape(10, 10), [0], [5], [[1], [2]])
    assert al.align_rows(logits.reshape(10, 10), [], [], []) == []
    with pytest.raises(_lib.M3Error, match="blank"):
        CtcAligner(10, blank=10, device="cpu")


# ---------------------------------------------------------------- StreamPool(timestamps=True): session time
class ScriptedDecoder:
    """What StreamPool(segment=True, timestamps=True[, rescore=True]) needs of a decoder: script[b] lists per chunk of slot b
    the frame inside the chunk at which the rule fires (or None); align() answers from `spans`, frames inside the SEGMENT."""

    def __init__(self, B, c, frame_ms=40, rescorer=None):
        from m3asr.align import Alignment
        self.Alignment = Alignment
        self.B, self.c, self.endpoint = B, c, EndpointConfig(rules=((False, 0, 10 * frame_ms),), frame_ms=frame_ms)
        self.aligner, self.rescorer = object(), rescorer
        self.log, self.chunks, self.fired = [], [0] * B, [None] * B
        self.script, self.hyp, self.spans, self.second = {}, {}, {}, {}

    def reset(self, slots=None, **kw):
        self.log.append(("reset", tuple(slots)))
        for b in slots:
            self.chunks[b], self.fired[b] = 0, None

    def step(self, window, valid):
        for b in range(self.B):
            if int(valid[b]) > 0:
                at = self.script[b].pop(0) if self.script.get(b) else None
                if at is not None and self.fired[b] is None:
                    self.fired[b] = self.chunks[b] * self.c + at
                self.chunks[b] += 1

    def endpoints(self, slots=None):
        return [EndpointInfo(0, -1, self.chunks[b] * self.c, 0, True, 0, 0) if self.fired[b] is None else
                EndpointInfo(1, self.fired[b], self.fired[b] + 1, 0, True, 0, self.fired[b]) for b in slots]

    def partial(self, slots=None):
        return [(self.hyp.get(b, ()), -1.0) for b in slots], [list(self.hyp.get(b, ())) for b in slots]

    def finish(self, slots=None):
        return [[(self.hyp.get(b, ()), -1.0), ((99,), -50.0)] for b in slots]

    def rescore(self, slots=None, detail=False):
        self.log.append(("rescore", tuple(slots)))
        return [(self.second[b], [(self.hyp[b], -1.0, -2.0, -3.0), (self.second[b], -1.5, -1.0, -2.5)]) for b in slots]

    def align(self, slots=None, tokens=None):
        self.log.append(("align", tuple(slots), tuple(tuple(t) for t in tokens)))
        out = []
        for b, toks in zip(slots, tokens):
            spans = self.spans.get((b, tuple(toks)))
            if spans is None:
                out.append(self.Alignment(list(toks), [], [], [], [], float("-inf"), [], False, [], [], []))
                continue
            s, e = [a for a, _ in spans], [z for _, z in spans]
            out.append(self.Alignment(list(toks), s, e, s, [0.5] * len(toks), -1.0, [], True, [40 * v for v in s], [40 * v for v in e],
                                      [40 * v for v in s]))
        return out


def _pool(dec, **kw):
    from m3asr.serve import StreamPool
    return StreamPool(dec, B=dec.B, chunk=dec.c, input_dim=2, segment=True, timestamps=True, **kw)


@pytest.mark.parametrize("frame_ms", [40, 30])
def test_times_are_session_times(frame_ms):
    """two sessions; session a is cut twice: the second segment's times are moved by the first segment's CHUNKS (2 c frames,
    not by the frame the rule fired at), in the endpoint config's frame_ms; one align call covers all slots that fired in a
    step and runs before either is restarted; an utterance CTC cannot align files times = None"""
    from m3asr.serve import Segment, TimedSegment
    c = 4
    dec = ScriptedDecoder(2, c, frame_ms)
    pool = _pool(dec)
    a, b = pool.open(), pool.open()
    sa, sb = pool.slot_of(a), pool.slot_of(b)
    dec.script[sa], dec.script[sb] = [None, 1, None, None, 3], [None, 2]
    dec.hyp[sa], dec.hyp[sb] = (7, 8), (5,)
    dec.spans[(sa, (7, 8))] = [(1, 3), (4, 5)]
    frames = torch.zeros(4 * c * 7 + 3, 2)
    pool.push(a, frames)
    pool.push(b, frames)
    pool.step()
    assert pool.segments(a) == [] and not [e for e in dec.log if e[0] == "align"]
    n_log = len(dec.log)
    pool.step()                                            # both fire in their second chunk
    assert dec.log[n_log:] == [("align", (sa, sb), ((7, 8), (5,))), ("reset", (sa,)), ("reset", (sb,))]
    seg, = pool.segments(a)
    assert isinstance(seg, TimedSegment) and seg.best is None and seg.scores is None
    assert Segment(*seg[:5]) == Segment(1, 0, (5 + 1) * frame_ms, [((7, 8), -1.0), ((99,), -50.0)], 5)
    assert seg.times == [(7, 1 * frame_ms, 3 * frame_ms, 0.5), (8, 4 * frame_ms, 5 * frame_ms, 0.5)]
    other, = pool.segments(b)
    assert other.times is None and other.nbest[0][0] == (5,)          # no alignment for (5,): filed all the same
    assert pool.offset_ms(a) == 2 * c * frame_ms
    for _ in range(3):
        pool.step()
    seg, = pool.segments(a)
    off = 2 * c
    assert seg.end_frame == off + 2 * c + 3
    assert seg.times == [(7, (off + 1) * frame_ms, (off + 3) * frame_ms, 0.5), (8, (off + 4) * frame_ms, (off + 5) * frame_ms, 0.5)]
    # close(timed=True): the open segment, offset by everything before it
    off = (2 + 3) * c
    rest, times = pool.close(a, timed=True)
    assert rest[0] == ((7, 8), -1.0) and times == [(7, (off + 1) * frame_ms, (off + 3) * frame_ms, 0.5),
                                                    (8, (off + 4) * frame_ms, (off + 5) * frame_ms, 0.5)]
    assert pool.close(b)[0][0] == (5,)                     # without timed= close() is what it was


def test_with_rescoring_the_second_pass_choice_is_aligned():
    from m3asr.serve import RescoredSegment, TimedSegment
    c = 4
    dec = ScriptedDecoder(1, c, rescorer=object())
    pool = _pool(dec, rescore=True)
    sid = pool.open()
    dec.script[0], dec.hyp[0], dec.second[0] = [0], (7, 8), (7, 9)
    dec.spans[(0, (7, 9))] = [(0, 1), (2, 4)]
    pool.push(sid, torch.zeros(4 * c * 2 + 3, 2))
    n_log = len(dec.log)
    pool.step()
    assert dec.log[n_log:] == [("rescore", (0,)), ("align", (0,), ((7, 9),)), ("reset", (0,))]
    seg, = pool.segments(sid)
    assert isinstance(seg, TimedSegment) and seg.best == (7, 9) and len(seg.scores) == 2
    assert RescoredSegment(*seg[:7]).best == (7, 9)
    assert seg.times == [(7, 0, 40, 0.5), (9, 80, 160, 0.5)]
    pool.step()
    (best, scores), times = pool.close(sid, rescored=True, timed=True)
    assert best == (7, 9) and times == [(7, (c + 0) * 40, (c + 1) * 40, 0.5), (9, (c + 2) * 40, (c + 4) * 40, 0.5)]


def test_timestamps_need_an_aligner_and_segments():
    from m3asr.serve import StreamPool
    dec = ScriptedDecoder(1, 4)
    with pytest.raises(_lib.M3Error, match="segment=True"):
        StreamPool(dec, B=1, chunk=4, input_dim=2, timestamps=True)
    dec.aligner = None
    with pytest.raises(_lib.M3Error, match="aligner"):
        StreamPool(dec, B=1, chunk=4, input_dim=2, segment=True, timestamps=True)
    dec.aligner = object()
    pool = StreamPool(dec, B=1, chunk=4, input_dim=2, segment=True)
    with pytest.raises(_lib.M3Error, match="timestamps=True"):
        pool.close(pool.open(), timed=True)
