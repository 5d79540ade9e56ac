"""Host side of endpoint detection and segmenting (no GPU): EndpointConfig, the m3_ctc_endpoint_* exports and descriptor
checks, WindowBuffer.rebase / AudioWindowBuffer.rebase against fresh buffers, and StreamPool(segment=True) over a scripted
decoder.  The kernel itself is tested in tests/test_ctc_endpoint_gpu.py."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import endpoint_ref
from conftest import ROOT
from m3asr import _lib, ops
from m3asr._lib import M3Error
from m3asr.decode import EndpointConfig, EndpointInfo
from m3asr.frontend import AudioWindowBuffer
from m3asr.serve import Segment, StreamPool, WindowBuffer


# ---------------------------------------------------------------- EndpointConfig
def test_ms_to_frames_is_a_ceiling():
    ep = EndpointConfig()
    assert [ep.frames(ms) for ms in (0, 1, 40, 41, 999, 1000, 1001)] == [0, 1, 1, 2, 25, 25, 26]
    assert ep.frames(999.5) == 25 and ep.frames(1000.0) == 25 and ep.frames(1000.5) == 26
    assert EndpointConfig(frame_ms=10).frames(1001) == 101


def test_defaults_and_descriptor():
    ep = EndpointConfig()
    assert ep.blank_threshold == 0.8 and ep.frame_ms == 40
    assert ep.frame_rules == ((False, 125, 0), (True, 25, 0), (False, 0, 500))
    assert ep.length_bound() == 500
    assert EndpointConfig(rules=((True, 1000, 0),)).length_bound() is None
    assert EndpointConfig(rules=((False, 0, 800), (False, 0, 400), (True, 0, 40))).length_bound() == 10
    d = ep.desc(7, blank=3)
    assert (d.B, d.blank, d.n_rules) == (7, 3, 3)
    assert d.log_blank_threshold == np.float32(math.log(0.8)) == np.float32(ep.log_blank_threshold)
    assert [(r.must_decoded, r.min_trailing, r.min_length) for r in d.rule] == [(0, 125, 0), (1, 25, 0), (0, 0, 500), (0, 0, 0)]
    assert ops.ctc_endpoint_state_size(d) == 7 * 8 * 4           # eight words per stream, whatever the session's length
    assert ops.ctc_endpoint_state_size(ep.desc(0)) == 0


@pytest.mark.parametrize("thr", [0.0, 0.3, 0.4999, 1.0, 1.5, -0.8, float("nan")])
def test_threshold_outside_half_to_one_is_refused(thr):
    with pytest.raises(ValueError, match="blank_threshold"):
        EndpointConfig(blank_threshold=thr)


def test_threshold_edges_are_accepted_by_the_library():
    for thr in (0.5, 0.75, 0.999999):
        assert EndpointConfig(blank_threshold=thr).desc(2).n_rules == 3


def test_rule_lists_that_are_refused():
    with pytest.raises(ValueError):
        EndpointConfig(rules=())
    with pytest.raises(ValueError):
        EndpointConfig(rules=((False, 0, 100),) * 5)
    with pytest.raises(ValueError):
        EndpointConfig(rules=((False, -40, 0),))


def _raw_desc(B=1, blank=0, n_rules=1, thr=math.log(0.8), rule=(0, 0, 10)):
    d = _lib.CtcEndpointDesc()
    d.B, d.blank, d.n_rules, d.log_blank_threshold = B, blank, n_rules, thr
    d.rule[0].must_decoded, d.rule[0].min_trailing, d.rule[0].min_length = rule
    return d


@pytest.mark.parametrize("kw,word", [(dict(B=-1), "B"), (dict(blank=-1), "blank"), (dict(n_rules=0), "n_rules"),
                                     (dict(n_rules=5), "n_rules"), (dict(thr=0.0), "threshold"), (dict(thr=-0.7), "threshold"),
                                     (dict(thr=float("nan")), "threshold"), (dict(rule=(0, -1, 0)), "rule"),
                                     (dict(rule=(0, 0, -1)), "rule"), (dict(rule=(2, 0, 0)), "rule")])
def test_library_refuses_bad_descriptors(kw, word):
    lib = _lib.load()
    assert lib.m3_ctc_endpoint_state_size(ctypes.byref(_raw_desc(**kw))) == 0
    assert word in _lib.last_error()
    # every entry point validates before it looks at a pointer
    assert lib.m3_ctc_endpoint_reset(ctypes.byref(_raw_desc(**kw)), None, 0, None) != 0
    assert lib.m3_ctc_endpoint_advance(ctypes.byref(_raw_desc(**kw)), None, 0, None, None, 4, 1, None, None) != 0
    assert lib.m3_ctc_endpoint_read(ctypes.byref(_raw_desc(**kw)), None, 0, None, None) != 0


def test_library_refuses_short_state_and_bad_shapes():
    lib = _lib.load()
    d = _raw_desc(B=3)
    assert lib.m3_ctc_endpoint_state_size(ctypes.byref(d)) == 96
    assert lib.m3_ctc_endpoint_reset(ctypes.byref(d), None, 95, None) != 0 and "95 bytes" in _lib.last_error()
    assert lib.m3_ctc_endpoint_advance(ctypes.byref(d), None, 96, None, None, -1, 1, None, None) != 0
    assert lib.m3_ctc_endpoint_advance(ctypes.byref(d), None, 96, None, None, 4, 0, None, None) != 0
    assert lib.m3_ctc_endpoint_advance(ctypes.byref(d), None, 96, None, None, 0, 1, None, None) == 0     # no frame, no launch
    assert lib.m3_ctc_endpoint_reset_slots(ctypes.byref(d), None, 96, None, 2, None) != 0
    assert lib.m3_ctc_endpoint_reset_slots(ctypes.byref(d), None, 96, None, 0, None) == 0


NEW_EXPORTS = ["m3_ctc_endpoint_advance", "m3_ctc_endpoint_read", "m3_ctc_endpoint_reset", "m3_ctc_endpoint_reset_slots",
               "m3_ctc_endpoint_state_size"]


def test_new_exports_and_unchanged_abi_version():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m3asr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(m3_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(n for n in declared if "_endpoint" in n) == NEW_EXPORTS
    assert _lib.load().m3_abi_version() == 10
    assert ctypes.sizeof(_lib.CtcEndpointDesc) == 16 + 4 * 12


def test_reference_rule_by_hand():
    """tests/endpoint_ref.py on a sequence small enough to follow: blank = 0, rules (after speech: 2 blanks) and (6 frames)."""
    thr = np.float32(math.log(0.8))
    ref = endpoint_ref.EndpointRef(0, thr, [(1, 2, 0), (0, 0, 6)])
    sure, weak = -0.01, -0.5
    ref.advance([[sure], [sure], [weak]], [[0], [0], [0]], 3)          # silence does not fire rule 1; a weak blank ends the run
    assert ref.info() == [3, 0, 0, -1, -1, 0, -1, 0]
    ref.advance([[-1.0], [sure]], [[4], [0]], 2)
    assert ref.info() == [5, 1, 1, 3, 3, 0, -1, 0]
    ref.advance([[thr]], [[0]], 1)                                     # exactly the threshold is not blank; rule 2 fires on length
    assert ref.info() == [6, 0, 1, 3, 3, 2, 5, 0]
    ref.advance([[-1.0]], [[4]], 1)                                    # latched
    assert ref.info() == [6, 0, 1, 3, 3, 2, 5, 0]
    ref.reset()
    assert ref.info() == list(endpoint_ref.FRESH) + [0]


# ---------------------------------------------------------------- rebase
def _drain(buf):
    out = []
    while buf.ready() > 0:
        win, n = buf.take()
        out.append((win.clone(), int(n), buf.ready()))
    return out


def _same_windows(a, b):
    assert len(a) == len(b)
    for (wa, na, ra), (wb, nb, rb) in zip(a, b):
        assert na == nb and ra == rb and torch.equal(wa, wb)


def _feed(bufs, data, rnd):
    """the same random pieces into every buffer; yields after each piece"""
    pos = 0
    while pos < len(data):
        n = min(rnd.randint(1, 90), len(data) - pos)
        for b in bufs:
            b.push(data[pos:pos + n])
        pos += n
        yield pos


@pytest.mark.parametrize("windows_before", [0, 1, 3])
@pytest.mark.parametrize("audio", [False, True])
def test_rebase_equals_a_fresh_buffer(audio, windows_before):
    """Random push sizes; after `windows_before` windows the buffer is rebased and a fresh buffer is pushed everything from
    the old input frame 4 c chunks on (sample 160 * 4 c chunks).  From there on both see the same pushes and must hand out
    the same windows, the same counts and the same ready() at every point, through end() and the short last window."""
    c, idim, rnd = 4, 3, random.Random(17 + windows_before)
    g = torch.Generator().manual_seed(5)
    if audio:
        data = torch.randint(-3000, 3000, (160 * 97 + 123,), generator=g, dtype=torch.int16)
        new, unit = (lambda: AudioWindowBuffer(c)), 160 * 4 * c
    else:
        data = torch.rand(97, idim, generator=g)
        new, unit = (lambda: WindowBuffer(c, idim)), 4 * c
    old, fresh, taken, split = new(), None, 0, int(len(data) * 0.6)
    feed = _feed([old], data[:split], rnd)
    for pos in feed:
        while taken < windows_before and old.ready() > 0:
            old.take()
            taken += 1
    while taken < windows_before:                    # the pieces so far held fewer windows: they are all there now
        old.take()
        taken += 1
    assert old.chunks == windows_before
    old.rebase()
    assert old.chunks == 0 and old.base == 0 and not old.ended
    fresh = new()
    fresh.push(data[unit * windows_before:split])
    assert old.total == fresh.total and old.ready() == fresh.ready()
    got, want = [], []
    for pos in _feed([old, fresh], data[split:], rnd):
        assert old.ready() == fresh.ready()
        if rnd.random() < 0.5:
            got += _drain(old)
            want += _drain(fresh)
    old.end()
    fresh.end()
    got += _drain(old)
    want += _drain(fresh)
    _same_windows(got, want)
    assert len(got) >= 2 and got[-1][1] < old.window and old.drained() and fresh.drained()


@pytest.mark.parametrize("audio", [False, True])
@pytest.mark.parametrize("tail", [0, 1, 6, 7, 9])
def test_rebase_after_end_with_a_short_tail(audio, tail):
    """end() first, then the rebase: `ended` is preserved, and what is left behaves as in a fresh, ended buffer: a tail of
    >= 7 frames behind the rebase point still runs as a short window, a shorter one never does."""
    c, idim = 4, 2
    g = torch.Generator().manual_seed(tail)
    frames = 4 * c * 2 + tail + (3 if tail == 0 else 0)             # two windows, then `tail` frames from the third's start
    if audio:
        data = torch.randint(-3000, 3000, (400 + 160 * (frames - 1),), generator=g, dtype=torch.int16)
        new, unit = (lambda: AudioWindowBuffer(c)), 160 * 4 * c
    else:
        data = torch.rand(frames, idim, generator=g)
        new, unit = (lambda: WindowBuffer(c, idim)), 4 * c
    old = new()
    old.push(data)
    old.end()
    old.take()
    old.take()
    old.rebase()
    assert old.ended and old.chunks == 0
    fresh = new()
    fresh.push(data[unit * 2:])
    fresh.end()
    assert old.total == fresh.total
    expect = tail if tail >= 7 else 0
    assert old.ready() == fresh.ready() == expect
    _same_windows(_drain(old), _drain(fresh))
    assert old.drained()
    with pytest.raises(ValueError):
        old.push(data[:1])
    # a rebase behind a short last window leaves nothing, as a fresh buffer that was pushed nothing
    if expect:
        old.rebase()
        assert (old.total, old.ready(), int(old.buf.shape[0])) == (0, 0, 0) and old.drained()


# ---------------------------------------------------------------- StreamPool(segment=True) over a scripted decoder
class ScriptedDecoder:
    """What StreamPool needs of a decoder, driven by a script: script[b] lists, per chunk that slot b runs after a reset,
    the frame (inside that chunk) at which a rule fires, or None; hyp[b] is the best hypothesis finish() reports."""

    def __init__(self, B, c, endpoint=EndpointConfig(rules=((False, 0, 400),))):
        self.B, self.c, self.endpoint = B, c, endpoint
        self.log, self.chunks, self.fired = [], [0] * B, [None] * B
        self.script, self.hyp, self.speech = {}, {}, {}

    def reset(self, slots=None, **kw):
        self.log.append(("reset", tuple(slots), kw))
        for b in slots:
            self.chunks[b], self.fired[b] = 0, None

    def step(self, window, valid):
        live = [b for b in range(self.B) if int(valid[b]) > 0]
        self.log.append(("step", tuple(live)))
        for b in live:
            at = self.script[b].pop(0) if self.script.get(b) else None
            if at is not None and self.fired[b] is None:
                self.fired[b] = self.chunks[b] * self.c + at
            self.chunks[b] += 1

    def endpoints(self, slots=None):
        self.log.append(("endpoints", tuple(slots)))
        out = []
        for b in slots:
            first, last = self.speech.get(b, (-1, -1))
            if self.fired[b] is None:
                out.append(EndpointInfo(0, -1, self.chunks[b] * self.c, 0, first >= 0, first, last))
            else:
                out.append(EndpointInfo(2, self.fired[b], self.fired[b] + 1, 3, first >= 0, first, last))
        return out

    def partial(self, slots=None):
        return [(self.hyp.get(b, ()), -1.0) for b in slots], [list(self.hyp.get(b, ())) for b in slots]

    def finish(self, slots=None):
        self.log.append(("finish", tuple(slots)))
        return [[(self.hyp.get(b, ()), -1.0 - self.chunks[b]), ((99,), -50.0)] for b in slots]


def _pool(dec, **kw):
    return StreamPool(dec, B=dec.B, chunk=dec.c, input_dim=2, segment=True, **kw)


def test_segments_offsets_and_times():
    c = 4
    dec = ScriptedDecoder(2, c)
    pool = _pool(dec)
    a, b = pool.open(), pool.open()
    sa, sb = pool.slot_of(a), pool.slot_of(b)
    # session a: fires in its 2nd chunk at frame 1 (frame 5 of the segment), then in the 3rd chunk after that at frame 3
    dec.script[sa] = [None, 1, None, None, 3]
    dec.hyp[sa], dec.speech[sa] = (7, 8), (2, 4)
    dec.script[sb] = []
    dec.hyp[sb] = (5,)
    frames = torch.arange(2 * (4 * c * 7 + 3), dtype=torch.float32).reshape(-1, 2)
    pool.push(a, frames)
    pool.push(b, frames)
    assert pool.offset_ms(a) == 0 and pool.segments(a) == []
    assert pool.step() == [a, b] and pool.segments(a) == []
    n_resets = sum(1 for e in dec.log if e[0] == "reset")
    assert pool.step() == [a, b]
    # one fire: only that slot was finished and reset, with nothing but the slot list (graph and LM setting are kept)
    assert dec.log[-3:] == [("endpoints", (sa, sb)), ("finish", (sa,)), ("reset", (sa,), {})]
    assert sum(1 for e in dec.log if e[0] == "reset") == n_resets + 1
    assert dec.chunks == [0, 2] if sa == 0 else dec.chunks == [2, 0]
    seg, = pool.segments(a)
    assert seg == Segment(2, 2 * 40, 5 * 40, [((7, 8), -3.0), ((99,), -50.0)], 5)
    assert pool.segments(a) == [] and pool.segments(b) == []                     # handed out once; b has none
    assert pool.offset_ms(a) == 2 * c * 40 and pool.offset_ms(b) == 0
    assert pool.slot_of(a) == sa and pool.streams[a][1].chunks == 0             # the sid survives, its buffer was rebased
    # the rebased buffer goes on at the session's input frame 4 c 2: the window of the next step starts there
    dec.speech[sa] = (0, 9)
    for _ in range(3):
        assert pool.step() == [a, b]
    assert torch.equal(pool.win[sa], frames[4 * c * 4: 4 * c * 4 + 4 * c + 3])
    seg, = pool.segments(a)
    assert (seg.rule, seg.start_ms, seg.end_ms, seg.end_frame) == (2, (8 + 0) * 40, (8 + 9 + 1) * 40, 8 + 2 * c + 3)
    assert seg.nbest[0] == ((7, 8), -4.0)
    assert pool.offset_ms(a) == (2 + 3) * c * 40
    # close: the n-best of the open segment, as without segmenting
    assert pool.close(b)[0][0] == (5,)
    assert pool.close(a)[0] == ((7, 8), -1.0)
    assert pool.free_slots() == 2
    with pytest.raises(KeyError):
        pool.segments(a)
    with pytest.raises(KeyError):
        pool.offset_ms(a)


def test_an_empty_segment_is_dropped_but_still_moves_the_session():
    c = 4
    dec = ScriptedDecoder(1, c)
    pool = _pool(dec)
    sid = pool.open()
    dec.script[0] = [2, None, 0]
    dec.hyp[0] = ()
    pool.push(sid, torch.zeros(4 * c * 4 + 3, 2))
    assert pool.step() == [sid]
    assert pool.segments(sid) == [] and pool.offset_ms(sid) == c * 40           # dropped; the slot was restarted all the same
    assert dec.log[-2:] == [("finish", (0,)), ("reset", (0,), {})]
    dec.hyp[0], dec.speech[0] = (3,), (-1, -1)                                  # a hypothesis without a non-blank argmax frame
    assert pool.step() == [sid] and pool.segments(sid) == []
    assert pool.step() == [sid]
    seg, = pool.segments(sid)
    assert (seg.start_ms, seg.end_ms, seg.end_frame) == (c * 40, (c + c + 0 + 1) * 40, c + c + 0)   # the whole segment


def test_idle_slots_are_not_asked_and_nothing_is_read_without_a_step():
    dec = ScriptedDecoder(3, 4)
    pool = _pool(dec)
    a, b = pool.open(), pool.open()
    pool.push(a, torch.zeros(4 * 4 + 3, 2))
    n = len(dec.log)
    assert pool.step() == [a]
    assert dec.log[n:] == [("step", (pool.slot_of(a),)), ("endpoints", (pool.slot_of(a),))]
    n = len(dec.log)
    assert pool.step() == [] and dec.log[n:] == []


def test_segmenting_needs_an_endpoint_config():
    class Plain:
        def step(self, window, valid):
            pass

        def reset(self, slots=None):
            pass

    with pytest.raises(M3Error, match="endpoint"):
        StreamPool(Plain(), B=1, chunk=4, input_dim=2, segment=True)
    dec = ScriptedDecoder(1, 4, endpoint=None)
    with pytest.raises(M3Error, match="endpoint"):
        _pool(dec)
    pool = StreamPool(dec, B=1, chunk=4, input_dim=2)                           # without segment= nothing changes
    sid = pool.open()
    with pytest.raises(ValueError):
        pool.segments(sid)
    with pytest.raises(ValueError):
        pool.offset_ms(sid)
    pool.push(sid, torch.zeros(19, 2))
    assert pool.step() == [sid] and not any(e[0] == "endpoints" for e in dec.log)


def test_the_length_rule_must_fit_max_frames():
    """min_length + c <= max_frames: before the firing chunk a slot stands below min_length, after it below min_length + c."""
    ep = EndpointConfig(rules=((True, 1000, 0), (False, 0, 400)))               # 10 frames
    assert ep.length_bound() == 10
    _pool(ScriptedDecoder(1, 4, endpoint=ep), max_frames=14)
    with pytest.raises(M3Error, match="max_frames"):
        _pool(ScriptedDecoder(1, 4, endpoint=ep), max_frames=13)
    _pool(ScriptedDecoder(1, 4, endpoint=EndpointConfig(rules=((True, 1000, 0),))), max_frames=4)   # no rule bounds the length
