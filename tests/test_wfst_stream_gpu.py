"""The graph search inside live sessions: StreamingCtcDecoder(graph=, wfst=) and StreamPool(words=True).

The yardstick is a stand-alone CtcWfstSearch fed the very logits and frame counts each step() of the decoder produced: the
decoder adds wiring, not arithmetic, so words, word frames, cost bits and reached_final must be equal -- with and without
blank-frame skipping, at every step, across a slot's reset and across the endpoints at which a pool cuts a session."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3asr._lib import M3Error
from m3asr.config import EncoderConfig
from m3asr.decode import EndpointConfig, StreamingCtcDecoder
from m3asr.engine import Engine
from m3asr.serve import StreamPool, WindowBuffer, WordSegment
from m3asr.weights import make_weights
from m3asr.wfst import CtcWfstSearch, DecodingGraph

C, MAXF, L_FRAMES, BEAM = 4, 16, 10, 4
LENGTH_RULE = EndpointConfig(rules=((False, 0, L_FRAMES * 40),))      # 10 frames: fires in a slot's third chunk
OPTS = dict(beam=12.0, max_active=300)
# A random model's blank is never sure: over V = 1434 its posterior lies between 0.0003 and 0.0010 on these inputs, median 0.00053,
# and the frames' best token is often the same from frame to frame.  A threshold at the median skips about half of the frames
# and makes the re-insert rule fire; the comparison itself holds at any threshold.
SKIP = 0.00055


@pytest.fixture(scope="module")
def engine():
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=C,
                        num_decoding_left_chunks=2)
    return Engine.from_state_dict(cfg, make_weights(cfg, seed=47), packed_rows=False)


@pytest.fixture(scope="module")
def graph(engine):
    """Every token a word, and a few words of two tokens with a cost, so that any CTC output spells something."""
    V = engine.cfg.output_dim
    lex = {t: [[t]] for t in range(1, V)}
    for k in range(40):
        lex[V + k] = [[1 + (7 * k) % (V - 1), 1 + (11 * k + 3) % (V - 1)]]
    return DecodingGraph.from_lexicon(lex, V, word_costs={w: 0.25 * (w % 4) for w in lex}).to("cuda")


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _same(got, want, what):
    assert got["words"] == want["words"] and got["frames"] == want["frames"] and got["status"] == want["status"], (what, got, want)
    assert _bits(got["cost"]) == _bits(want["cost"]) and got["reached_final"] == want["reached_final"], (what, got, want)


def _tap(dec, rec):
    """record (logits, n_out) of every step() of `dec`, as device clones"""
    orig = dec.step

    def step(window, valid, n_out=None, use_graph=True):
        logits = orig(window, valid, n_out, use_graph)
        dec.st.eng.stream.synchronize()
        rec.append((logits.clone(), dec.n_out.clone()))
        return logits

    dec.step = step
    return dec


def _feed(dec, bufs, win):
    """one step of `dec` over the slots whose WindowBuffer has a window ready -> whether any had"""
    valid = torch.zeros(len(bufs), dtype=torch.int32)
    for b, buf in enumerate(bufs):
        if buf is not None and buf.ready() > 0:
            _, valid[b] = buf.take(out=win[b])
    if int(valid.sum()) > 0:
        dec.step(win, valid)
    return int(valid.sum()) > 0


@pytest.mark.parametrize("skip", [None, SKIP])
def test_decoder_words_equal_a_search_fed_the_same_logits(engine, graph, skip):
    idim = engine.cfg.input_dim
    g = torch.Generator().manual_seed(5)
    feats = [torch.rand(4 * C * 4 + 3, idim, generator=g), torch.rand(4 * C * 2 + 3, idim, generator=g)]
    rec = []
    dec = _tap(StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, graph=graph, wfst=dict(OPTS, blank_skip=skip)), rec)
    alone = CtcWfstSearch(graph, 2, MAXF, blank_skip=skip, **OPTS)
    assert (dec.wfst.skip is None) == (skip is None) and dec.wfst.desc.max_frames == MAXF
    bufs = [WindowBuffer(C, idim), None]
    bufs[0].push(feats[0])
    win = torch.zeros(2, 4 * C + 3, idim)
    steps = 0
    while _feed(dec, bufs, win):
        alone.advance(*rec[-1])
        got, want = dec.words(detail=True), alone.result(final=False, detail=True)
        for b in (0, 1):
            _same(got[b], want[b], "step %d slot %d" % (steps, b))
        steps += 1
        if steps == 1:                                                 # the second session starts one step later
            bufs[1] = WindowBuffer(C, idim)
            bufs[1].push(feats[1])
    assert steps == 4 and [n.tolist() for _, n in rec] == [[C, 0], [C, C], [C, C], [C, 0]]
    got, want = dec.words(final=True, detail=True), alone.result(final=True, detail=True)
    for b in (0, 1):
        _same(got[b], want[b], "final, slot %d" % b)
    part = alone.result(final=False)
    assert dec.words(slots=[1, 0]) == [part[1], part[0]] and dec.words(slots=[]) == []
    assert len(want[0]["words"]) > 0, "the random model spells nothing: the comparison would be empty"
    if skip is not None:
        counts = dec.wfst.frames()
        print("frames (seen, decoded):", counts)
        assert counts == alone.frames() and [s for s, _ in counts] == [4 * C, 2 * C]
        assert 0 < sum(k for _, k in counts) < 6 * C, "the threshold skips nothing or everything: choose another"
        assert all(0 <= f < 4 * C for f in want[0]["frames"])


def test_decode_words_runs_whole_utterances(engine, graph):
    idim = engine.cfg.input_dim
    g = torch.Generator().manual_seed(6)
    feat = torch.rand(2, 4 * C * 3 + 3, idim, generator=g)
    lens = torch.tensor([4 * C * 3 + 3, 4 * C + 9], dtype=torch.int32)
    rec = []
    dec = _tap(StreamingCtcDecoder(engine.streaming(2, MAXF), beam=BEAM, graph=graph, wfst=dict(OPTS, blank_skip=SKIP)), rec)
    got = dec.decode_words(feat, lens)
    alone = CtcWfstSearch(graph, 2, MAXF, blank_skip=SKIP, **OPTS)
    for logits, n_out in rec:
        alone.advance(logits, n_out)
    assert got == alone.result(final=True) and len(rec) == 3 and sum(len(w) for w in got) > 0


def test_a_slot_reset_leaves_the_other_slots_words_alone(engine, graph):
    idim = engine.cfg.input_dim
    g = torch.Generator().manual_seed(7)
    feats = [torch.rand(4 * C * 4 + 3, idim, generator=g) for _ in range(2)]
    rec = []
    dec = _tap(StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, graph=graph, wfst=dict(OPTS, blank_skip=SKIP)), rec)
    bufs = [WindowBuffer(C, idim), WindowBuffer(C, idim)]
    win = torch.zeros(2, 4 * C + 3, idim)
    for b in (0, 1):
        bufs[b].push(feats[b])
    fresh = dec.words(detail=True)[0]
    assert _feed(dec, bufs, win) and _feed(dec, bufs, win)
    before = dec.words(detail=True)
    dec.reset(slots=[0])
    after = dec.words(detail=True)
    _same(after[1], before[1], "slot 1 across the reset of slot 0")
    _same(after[0], fresh, "slot 0 after its reset")
    assert dec.wfst.frames() == [(0, 0), (2 * C, dec.wfst.frames()[1][1])]
    bufs[0] = WindowBuffer(C, idim)
    bufs[0].push(feats[0][:4 * C * 2 + 3])
    assert _feed(dec, bufs, win) and _feed(dec, bufs, win)
    # slot 1 saw four chunks in a row; slot 0 its first two chunks again, from a fresh state
    alone = CtcWfstSearch(graph, 2, MAXF, blank_skip=SKIP, **OPTS)
    for i, (logits, n_out) in enumerate(rec):
        if i == 2:
            alone.reset(slots=[0])
        alone.advance(logits, n_out)
    got, want = dec.words(final=True, detail=True), alone.result(final=True, detail=True)
    for b in (0, 1):
        _same(got[b], want[b], "slot %d at the end" % b)
    first_two = CtcWfstSearch(graph, 2, MAXF, blank_skip=SKIP, **OPTS)
    for logits, n_out in rec[2:]:
        first_two.advance(logits, n_out)
    _same(got[0], first_two.result(final=True, detail=True)[0], "slot 0 equals a search that only saw the frames after its reset")


def test_a_pool_session_across_endpoints_files_word_segments_in_session_time(engine, graph):
    idim = engine.cfg.input_dim
    g = torch.Generator().manual_seed(21)
    feat = torch.rand(4 * C * 7 + 3, idim, generator=g)                 # seven chunks: two segments of three, one chunk left open
    rec = []
    dec = _tap(StreamingCtcDecoder(engine.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE, graph=graph,
                                   wfst=dict(OPTS, blank_skip=SKIP)), rec)
    prefixes, finish = [], dec.finish
    dec.finish = lambda slots=None, detail=False: prefixes.append(finish(slots=slots, detail=detail)) or prefixes[-1]
    pool = StreamPool(dec, segment=True, words=True)
    sid = pool.open()
    pool.push(sid, feat)
    segs = []
    while pool.step():
        segs += pool.segments(sid)
    assert len(rec) == 7 and pool.offset_ms(sid) == 6 * C * 40 and len(prefixes) == 2
    alone = CtcWfstSearch(graph, 2, MAXF, blank_skip=SKIP, **OPTS)
    want = []
    for j in range(2):
        alone.reset()
        for logits, n_out in rec[3 * j:3 * j + 3]:
            alone.advance(logits, n_out)
        want.append(alone.result(final=True, detail=True)[0])
    # a segment is filed when its best prefix or its word list is not empty
    filed = [j for j in range(2) if (prefixes[j][0] and len(prefixes[j][0][0][0]) > 0) or want[j]["words"]]
    print("segments filed:", filed, [w["words"] for w in want], [w["frames"] for w in want])
    assert len(segs) == len(filed) and all(isinstance(s, WordSegment) for s in segs), segs
    assert 1 in filed and want[1]["words"], "the second segment has no words: its session times would not be checked"
    for j, seg in zip(filed, segs):
        w, off = want[j], 3 * C * j
        assert seg.words == w["words"] and seg.word_ms == [(off + f) * 40 for f in w["frames"]], (j, seg, w)
        assert all(off * 40 <= ms < (off + 3 * C) * 40 for ms in seg.word_ms), (j, seg.word_ms)
        assert _bits(seg.cost) == _bits(w["cost"]) and seg.reached_final == w["reached_final"] and seg.end_frame == off + L_FRAMES - 1
        assert seg.nbest == prefixes[j][0]
    # the open segment: one chunk behind the second cut
    alone.reset()
    alone.advance(*rec[6])
    w = alone.result(final=False, detail=True)[0]
    assert pool.words(sid) == (w["words"], [(6 * C + f) * 40 for f in w["frames"]])
    pool.close(sid)


def test_refusals(engine, graph):
    st = lambda: engine.streaming(2, MAXF, independent=True)           # noqa: E731
    plain = StreamingCtcDecoder(st(), beam=BEAM, endpoint=LENGTH_RULE)
    assert plain.wfst is None and plain.graph is None
    with pytest.raises(M3Error, match="graph"):
        plain.words()
    with pytest.raises(M3Error, match="graph"):
        plain.decode_words(torch.zeros(2, 19, engine.cfg.input_dim), torch.tensor([19, 19]))
    with pytest.raises(M3Error, match="graph"):
        StreamPool(plain, segment=True, words=True)
    with pytest.raises(M3Error, match="without graph"):
        StreamingCtcDecoder(st(), beam=BEAM, wfst=dict(OPTS))
    small = DecodingGraph.from_lexicon({1: [1]}, 5)
    with pytest.raises(M3Error, match="V = 5"):
        StreamingCtcDecoder(st(), beam=BEAM, graph=small.to("cuda"))
    host = DecodingGraph.from_lexicon({1: [1]}, engine.cfg.output_dim)
    with pytest.raises(M3Error, match="not on a device"):
        StreamingCtcDecoder(st(), beam=BEAM, graph=host)
    host.dev = torch.from_numpy(host.image)
    with pytest.raises(M3Error, match="is on cpu"):
        StreamingCtcDecoder(st(), beam=BEAM, graph=host)
    with pytest.raises(M3Error, match="unknown options"):
        StreamingCtcDecoder(st(), beam=BEAM, graph=graph, wfst=dict(lattice=True))
    with pytest.raises(M3Error, match="blank_skip"):
        StreamingCtcDecoder(st(), beam=BEAM, graph=graph, wfst=dict(blank_skip=1.0))
    dec = StreamingCtcDecoder(st(), beam=BEAM, endpoint=LENGTH_RULE, graph=graph)
    for kw in (dict(rescore=True), dict(timestamps=True)):
        with pytest.raises(M3Error, match="words=True"):
            StreamPool(dec, segment=True, words=True, **kw)
    with pytest.raises(M3Error, match="words=True"):
        pool = StreamPool(dec, segment=True)
        pool.words(pool.open())
    with pytest.raises(ValueError, match="slots"):
        dec.words(slots=[2])
