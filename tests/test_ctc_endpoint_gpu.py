"""Endpoint detection on the device (m3_ctc_endpoint_*, csrc/ctc_beam.hip) and what is built on it: StreamingCtcDecoder(endpoint=),
StreamPool(segment=True).

Kernel cases run on synthetic (top_logp, top_idx) and must equal tests/endpoint_ref.py, the rule frame by frame in plain
Python, EXACTLY: the state is integers.  Entries 1 .. k-1 of every frame hold a confident blank, so a kernel that judged a
frame by anything but entry 0 would count blanks that are none.  End to end a small slot-mode streaming engine (c = 4, B = 2)
is cut by a length rule, and every segment must equal, tokens and scores, a fresh session fed that segment's frames.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import endpoint_ref
import guarded
from m3asr import ops
from m3asr._lib import M3Error
from m3asr.config import EncoderConfig
from m3asr.decode import EndpointConfig, StreamingCtcDecoder
from m3asr.engine import Engine
from m3asr.serve import StreamPool, WindowBuffer
from m3asr.weights import make_weights

B, BLANK, V = 5, 2, 11
THR = np.float32(math.log(0.8))
SURE, WEAK = np.float32(-0.01), np.float32(-0.5)          # a blank above the threshold, and one below


def _topk(idx0, logp0, k):
    """(top_logp, top_idx) (B, T, k) float32 / int32 whose entry 0 is given; every other entry is a confident blank."""
    idx0, logp0 = np.asarray(idx0, dtype=np.int32), np.asarray(logp0, dtype=np.float32)
    lp = np.full(idx0.shape + (k,), SURE, dtype=np.float32)
    ix = np.full(idx0.shape + (k,), BLANK, dtype=np.int32)
    lp[..., 0], ix[..., 0] = logp0, idx0
    return lp, ix


def _mixed(T, seed):
    """Five streams of T frames that differ in kind: all tokens; tokens, then confident blanks; only confident blanks; a
    random mix of tokens, confident and weak blanks; blanks exactly at the threshold (which are not blank frames) with a
    token late."""
    rng = np.random.default_rng(seed)
    idx = np.full((B, T), BLANK, dtype=np.int32)
    lp = np.full((B, T), SURE, dtype=np.float32)
    tok = lambda n: rng.choice([v for v in range(V) if v != BLANK], n)
    idx[0], lp[0] = tok(T), -1.5
    idx[1, :min(20, T)], lp[1, :min(20, T)] = tok(min(20, T)), -0.7
    kind = rng.integers(0, 3, T)
    idx[3] = np.where(kind == 0, tok(T), BLANK)
    lp[3] = np.where(kind == 1, SURE, WEAK)
    lp[4] = THR
    if T > 100:
        idx[4, 100] = 7
    return idx, lp


class Device:
    """The detector's state on the device and the calls on it."""

    def __init__(self, rules, k, thr=THR, state=None):
        self.rules, self.k, self.thr = rules, k, thr
        self.desc = ops.ctc_endpoint_desc(B, BLANK, float(thr), rules)
        self.state = torch.empty(ops.ctc_endpoint_state_size(self.desc), dtype=torch.uint8, device="cuda") if state is None else state
        ops.ctc_endpoint_reset(self.desc, self.state)
        self.calls = []

    def advance(self, idx0, logp0, n_frames):
        lp, ix = _topk(idx0, logp0, self.k)
        self.calls.append((lp, ix, np.clip(np.asarray(n_frames), 0, lp.shape[1])))
        ops.ctc_endpoint_advance(self.desc, self.state, torch.from_numpy(lp).cuda(), torch.from_numpy(ix).cuda(),
                                 torch.tensor([int(v) for v in n_frames], dtype=torch.int32, device="cuda"))

    def info(self):
        return ops.ctc_endpoint_read(self.desc, self.state).cpu().tolist()

    def want(self):
        return endpoint_ref.run(BLANK, self.thr, self.rules, self.calls, B)

    def check(self):
        got, want = self.info(), self.want()
        assert got == want, "\ndevice %s\nref    %s" % (got, want)
        return got


def _in_pieces(dev, idx, lp, sizes):
    pos = 0
    for n in sizes:
        dev.advance(idx[:, pos:pos + n], lp[:, pos:pos + n], [n] * B)
        pos += n
    assert pos == idx.shape[1]


CHUNKINGS = {"one call": [130], "16s": [16] * 8 + [2], "1s": [1] * 130, "64+65+1": [64, 65, 1], "65+64+1": [65, 64, 1]}
# rules that fire at different frames in different streams, and rules that never fire (all 130 frames are consumed and
# first / last speech, the trailing run and the frame count cross the 64-lane boundary)
RULESETS = {"firing": [(0, 40, 0), (1, 7, 0), (0, 0, 120)], "silent": [(0, 500, 0), (1, 131, 10), (0, 0, 131)]}


@pytest.fixture(scope="module")
def mixed130():
    return _mixed(130, seed=3)


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("rules", sorted(RULESETS))
def test_chunking_invariance(mixed130, rules, k):
    idx, lp = mixed130
    infos = {}
    for name, sizes in CHUNKINGS.items():
        dev = Device(RULESETS[rules], k)
        _in_pieces(dev, idx, lp, sizes)
        infos[name] = dev.check()
    assert all(v == infos["one call"] for v in infos.values()), infos
    fired = [row[5] for row in infos["one call"]]
    if rules == "firing":                        # every rule is seen, at frames before, at and behind the iteration boundary
        assert fired == [3, 2, 1, 3, 3] and [row[6] for row in infos["one call"]] == [119, 26, 39, 119, 119]
    else:
        assert fired == [0] * B and [row[0] for row in infos["one call"]] == [130] * B
        assert infos["one call"][0][3:5] == [0, 129] and infos["one call"][1][1:5] == [110, 1, 0, 19]
        assert infos["one call"][2][1:5] == [130, 0, -1, -1] and infos["one call"][4][1:5] == [0, 1, 100, 100]


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("P", [63, 64])
def test_firing_on_lane_63_and_on_lane_0_of_the_second_iteration(P, k):
    """One 130-frame call.  Frame P ends streams 0, 1 and 3: stream 0 (silence) and 3 (tokens throughout) by the length rule,
    stream 1 by five trailing blanks behind a token at frame P - 5 (rule 1 wins where both hold).  Stream 2 ends early,
    stream 4 has 40 real frames and does not end."""
    T = 130
    idx = np.full((B, T), BLANK, dtype=np.int32)
    lp = np.full((B, T), SURE, dtype=np.float32)
    idx[1, P - 5] = 4
    idx[2, 3] = 5
    idx[3] = 9
    dev = Device([(1, 5, 0), (0, 0, P + 1)], k)
    dev.advance(idx, lp, [T, T, T, T, 40])
    got = dev.check()
    assert [(r[5], r[6]) for r in got] == [(2, P), (1, P), (1, 8), (2, P), (0, -1)]
    assert got[0][:5] == [P + 1, P + 1, 0, -1, -1] and got[1][:5] == [P + 1, 5, 1, P - 5, P - 5]
    assert got[3][:5] == [P + 1, 0, 1, 0, P] and got[4][:5] == [40, 40, 0, -1, -1]


@pytest.mark.parametrize("k", [1, 10])
def test_firing_on_the_first_frame_of_a_later_call(k):
    idx, lp = _mixed(70, seed=8)
    dev = Device([(0, 0, 17), (1, 60, 0)], k)
    dev.advance(idx[:, :16], lp[:, :16], [16] * B)
    assert [r[5] for r in dev.check()] == [0] * B
    dev.advance(idx[:, 16:], lp[:, 16:], [54] * B)
    got = dev.check()
    assert [(r[5], r[6]) for r in got] == [(1, 16)] * B


@pytest.mark.parametrize("k", [1, 10])
def test_padding_rows_and_idle_slots(k):
    """n_frames = [20, 7, 0, 25, -3] of T_chunk = 20 rows: the rows past a stream's count hold confident blanks and must
    not count (stream 1 would reach ten trailing blanks and end), counts are clamped to [0, T_chunk], and the streams with
    no frame keep their state word for word.  State, inputs and info sit in guarded memory."""
    rules, T = [(0, 10, 0)], 20
    state = guarded.flat_out((B * 32,), torch.uint8)
    dev = Device(rules, k, state=state.view)
    idx = np.full((B, T), BLANK, dtype=np.int32)
    lp = np.full((B, T), SURE, dtype=np.float32)
    idx[:, 2] = 6                                                     # every stream: a token at frame 2 ...
    dev.advance(idx[:, :4], lp[:, :4], [4] * B)                       # ... so that no state is the fresh one
    before = state.view.cpu().clone()
    lp_h, ix_h = _topk(idx, lp, k)
    n_frames = [20, 7, 0, 25, -3]
    dev.calls.append((lp_h, ix_h, np.clip(n_frames, 0, T)))
    g_lp = guarded.flat_in(torch.from_numpy(lp_h))                    # a frame read past the end: NaN is no blank, and
    g_ix = guarded.flat_in(torch.from_numpy(ix_h), int_guard=BLANK + 1)     # the guard token is speech
    g_info = guarded.flat_out((B, 8), torch.int32)
    ops.ctc_endpoint_advance(dev.desc, state.view, g_lp.view, g_ix.view, torch.tensor(n_frames, dtype=torch.int32, device="cuda"))
    ops.ctc_endpoint_read(dev.desc, state.view, g_info.view)
    got = g_info.view.cpu().tolist()
    assert got == dev.want()
    assert [r[5] for r in got] == [1, 0, 0, 1, 0] and got[1][:5] == [11, 4, 1, 2, 6] and got[0][6] == 16
    after = state.view.cpu()
    for b in (2, 4):
        assert torch.equal(after[32 * b: 32 * b + 32], before[32 * b: 32 * b + 32]), b
    state.check("endpoint state")
    g_info.check("endpoint info")
    assert not bool(g_info.untouched().any())


@pytest.mark.parametrize("k", [1, 10])
def test_latch_threshold_and_must_decoded(k):
    """Stream 0: a blank at exactly the threshold is no blank frame (it ends the run, and is no speech).  Stream 1: blanks
    below the threshold reset the run without setting `decoded`.  Stream 2: must_decoded holds rule 1 back through a long
    silence until the first token, then three blanks end it.  Stream 3: rule 2 (silence only) ends it.  After the fire a
    further advance, tokens and all, changes nothing."""
    T = 30
    idx = np.full((B, T), BLANK, dtype=np.int32)
    lp = np.full((B, T), SURE, dtype=np.float32)
    lp[0, 5], lp[0, 12] = THR, np.nextafter(THR, np.float32(0))       # frame 5 is not blank, frame 12 just is
    lp[1, 4:T:6] = WEAK
    idx[2, 20] = 3
    lp[4] = WEAK
    idx[4, 7] = 8
    dev = Device([(1, 3, 0), (0, 8, 0)], k)
    dev.advance(idx, lp, [T] * B)
    got = dev.check()
    # stream 0: run 0..4 (5), frame 5 resets, run 6.. reaches 8 at frame 13; stream 1: never 8 in a row; stream 2: frame 23
    assert [(r[5], r[6]) for r in got] == [(2, 13), (0, -1), (2, 7), (2, 7), (0, -1)]
    assert got[0][:5] == [14, 8, 0, -1, -1] and got[1][:5] == [30, 1, 0, -1, -1] and got[4][:5] == [30, 0, 1, 7, 7]
    dev2 = Device([(1, 3, 0), (0, 100, 0)], k)                        # without the silence rule stream 2 waits for its token
    dev2.advance(idx, lp, [T] * B)
    got2 = dev2.check()
    assert [(r[5], r[6]) for r in got2] == [(0, -1), (0, -1), (1, 23), (0, -1), (0, -1)]
    assert got2[2][:5] == [24, 3, 1, 20, 20]
    # latched: more frames, more tokens, nothing moves (the reference latches in the same way)
    idx[:] = 9
    for d, g in ((dev, got), (dev2, got2)):
        d.advance(idx, lp, [T] * B)
        now = d.check()
        for b in range(B):
            assert (now[b] == g[b]) == (g[b][5] != 0), b


def test_reset_slots_resets_only_the_listed_streams():
    idx, lp = _mixed(40, seed=4)
    dev = Device([(0, 0, 30)], 3)
    dev.advance(idx, lp, [40] * B)
    before = dev.check()
    assert all(r[5] == 1 for r in before)
    ops.ctc_endpoint_reset(dev.desc, dev.state, torch.tensor([1, 3, 7, -2], dtype=torch.int32, device="cuda"))
    after = dev.info()
    fresh = list(endpoint_ref.FRESH) + [0]
    assert after == [before[0], fresh, before[2], fresh, before[4]]
    dev.advance(idx[:, :5], lp[:, :5], [5] * B)                       # the restarted ones go on, the others stay latched
    now = dev.info()
    assert [r[0] for r in now] == [30, 5, 30, 5, 30] and now[0] == before[0]
    ops.ctc_endpoint_reset(dev.desc, dev.state)
    assert dev.info() == [fresh] * B


# ---------------------------------------------------------------- end to end
C, MAXF, L_FRAMES, BEAM = 4, 16, 10, 4
LENGTH_RULE = EndpointConfig(rules=((False, 0, L_FRAMES * 40),))      # 10 frames: fires in a slot's third chunk


@pytest.fixture(scope="module")
def engine():
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=C,
                        num_decoding_left_chunks=2)
    return Engine.from_state_dict(cfg, make_weights(cfg, seed=47), packed_rows=False)


def _alone(dec, b, frames, collect=None):
    """A fresh session in slot b of `dec`, fed exactly `frames` (never ended) -> (n-best, EndpointInfo)."""
    dec.reset(slots=[b])
    buf = WindowBuffer(C, frames.shape[1])
    buf.push(frames)
    win = torch.zeros(dec.beam.B, 4 * C + 3, frames.shape[1])
    while buf.ready() > 0:
        valid = torch.zeros(dec.beam.B, dtype=torch.int32)
        _, valid[b] = buf.take(out=win[b])
        logits = dec.step(win, valid)
        if collect is not None:
            dec.st.eng.stream.synchronize()
            collect.append(logits[b].cpu().clone())
    return dec.finish(slots=[b])[0], dec.endpoints(slots=[b])[0]


def test_a_long_stream_is_cut_into_segments_that_equal_fresh_sessions(engine):
    """Two sessions of 13 and 11 chunks (52 and 44 output frames, both > 2 max_frames = 32), the second starting two steps
    later, through StreamPool(segment=True) with the length rule alone: a segment every three chunks.  Segment j of a
    session must equal a fresh session fed the 4 c 3 + 3 feature frames from input frame 4 c 3 j on: n-best (prefixes and
    scores, exactly), and its times must be that session's first / last speech frame moved by the offset."""
    idim = engine.cfg.input_dim
    g = torch.Generator().manual_seed(21)
    feats = [torch.rand(4 * C * 13 + 3, idim, generator=g), torch.rand(4 * C * 11 + 3, idim, generator=g)]
    per_seg = -(-L_FRAMES // C)                                       # chunks a slot runs until the rule fires
    assert L_FRAMES % C != 0 and L_FRAMES + C <= MAXF and per_seg == 3
    dec = StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE)
    pool = StreamPool(dec, segment=True)
    sids, segs, sent, step = {}, {0: [], 1: []}, {0: 0, 1: 0}, 0
    start, pieces = {0: 0, 1: 2}, [23, 7, 40]
    offsets = {0: [], 1: []}
    while True:
        assert step < 100, "schedule does not end"
        for i in (0, 1):
            if step >= start[i] and i not in sids:
                sids[i] = pool.open()
            if i in sids and sent[i] < feats[i].shape[0]:
                n = min(pieces[(step + i) % 3], feats[i].shape[0] - sent[i])
                pool.push(sids[i], feats[i][sent[i]:sent[i] + n])
                sent[i] += n
        live = pool.step()
        for i in sids:
            got = pool.segments(sids[i])
            segs[i] += got
            offsets[i] += [pool.offset_ms(sids[i])] * len(got)
        if not live and all(sent[i] == feats[i].shape[0] for i in (0, 1)):
            break
        step += 1
    assert [pool.slot_of(sids[i]) for i in (0, 1)] == [0, 1]           # the sids survived every fire, in their slots
    assert dec.st.positions().tolist() == [C, 2 * C]                   # 13 = 4 * 3 + 1 chunks, 11 = 3 * 3 + 2
    assert [pool.offset_ms(sids[i]) for i in (0, 1)] == [4 * per_seg * C * 40, 3 * per_seg * C * 40]
    last = [pool.close(sids[i]) for i in (0, 1)]
    # the yardstick: a second decoder on the same engine, one fresh session per segment
    ref = StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE)
    n_seen = 0
    for i, n_segs in ((0, 4), (1, 3)):
        want = []
        for j in range(n_segs):
            f0 = 4 * C * per_seg * j
            nbest, info = _alone(ref, i, feats[i][f0:f0 + 4 * C * per_seg + 3])
            assert (info.rule, info.frame, info.frames) == (1, L_FRAMES - 1, L_FRAMES)
            off = per_seg * C * j
            if len(nbest[0][0]) > 0:                                  # a segment without a token is dropped
                first = info.first_speech if info.first_speech >= 0 else 0
                lastf = info.last_speech if info.last_speech >= 0 else info.frame
                want.append((1, (off + first) * 40, (off + lastf + 1) * 40, nbest, off + L_FRAMES - 1))
        assert [tuple(s) for s in segs[i]] == want, (i, segs[i], want)
        assert offsets[i] == [(s[4] - (L_FRAMES - 1) + per_seg * C) * 40 for s in want]
        n_seen += len(want)
        # the open segment at close(): what is left behind the last cut
        f0 = 4 * C * per_seg * n_segs
        nbest, info = _alone(ref, i, feats[i][f0:])
        assert last[i] == nbest and info.rule == 0
    assert n_seen >= 4, "the random model decodes nothing: the comparison would be empty"


def test_without_segmenting_the_same_stream_runs_past_max_frames(engine):
    """The session that segment=True carries to its end is refused by the streaming state after max_frames / c chunks: the
    wrapper raises on the host, before anything is launched."""
    g = torch.Generator().manual_seed(21)
    feat = torch.rand(4 * C * 13 + 3, engine.cfg.input_dim, generator=g)
    dec = StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE)
    pool = StreamPool(dec)
    sid = pool.open()
    pool.push(sid, feat)
    for _ in range(MAXF // C):
        assert pool.step() == [sid]
    with pytest.raises(M3Error, match="max_frames"):
        pool.step()
    assert dec.endpoints()[0].rule == 1                                # the detector saw the endpoint; nobody acted on it


def test_decoder_endpoints_follow_the_rule_on_real_logits(engine):
    """StreamingCtcDecoder(endpoint=) against endpoint_ref on the top-k of the logits each step returned (the detector
    reuses the beam search's top-k); a stream that is idle in a step does not move; reset(slots=) restarts one stream;
    without a config nothing is allocated and endpoints() raises."""
    idim = engine.cfg.input_dim
    ep = EndpointConfig(blank_threshold=0.5, rules=((True, 80, 0), (False, 0, 560)))
    dec = StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=ep)
    g = torch.Generator().manual_seed(33)
    logits = []
    _, info = _alone(dec, 1, torch.rand(4 * C * 4 + 3, idim, generator=g), collect=logits)
    ref = endpoint_ref.EndpointRef(0, ep.log_blank_threshold, ep.frame_rules)
    for lg in logits:
        lp, ix = ops.ctc_topk(lg.cuda(), BEAM)
        ref.advance(lp.cpu().numpy(), ix.cpu().numpy(), C)
    both = dec.endpoints()
    assert list(both[1]) == [ref.fired_rule, ref.fired_frame, ref.frames, ref.trailing_blank, bool(ref.decoded),
                             ref.first_speech, ref.last_speech]
    assert both[1] == info and both[1].rule != 0
    assert tuple(both[0]) == (0, -1, 0, 0, False, -1, -1)             # slot 0 was idle throughout
    dec.reset(slots=[1])
    assert tuple(dec.endpoints(slots=[1])[0]) == (0, -1, 0, 0, False, -1, -1)
    plain = StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM)
    assert plain.endpoint is None and not hasattr(plain, "estate")
    with pytest.raises(M3Error, match="endpoint"):
        plain.endpoints()
    with pytest.raises(M3Error, match="endpoint"):
        StreamPool(plain, segment=True)
    with pytest.raises(M3Error, match="max_frames"):                  # the default 20 s rule needs 500 + c frames
        StreamPool(StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=EndpointConfig()),
                   segment=True)
