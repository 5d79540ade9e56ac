"""CTC forced alignment on the device: m3_ctc_align_emit / m3_ctc_align_path (csrc/ctc_align.hip), CtcAligner,
CtcDecoder.align, StreamingCtcDecoder(aligner=), StreamPool(timestamps=True) and the --timestamps command lines.

Yardsticks.  The path stage is exact arithmetic: every output must equal the float32 restatement (tests/ctc_align_ref.py) bit
for bit, in guarded memory, and on emissions that are multiples of 1/4 the float64 restatement too.  The emit stage carries
the only rounding: float64 is the truth, e32 the error of the float32 restatement on the same rows, and the device must lie
within b = max(8 e32, 1e-5); every comparison prints its error, e32 and the bound before it asserts (run with -s).  End to
end, the device path is optimal under emissions that are off by at most b and summed in float32 over T frames, so its float64
re-score lies within 2 T b + 2 T ulp32(|optimum|) of the float64 optimum.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_align_ref as R
import guarded
from m3asr import ops
from m3asr._lib import M3Error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------- 1. the path stage, bit for bit
def _run_path(cases, max_frames, max_tokens, blank=0, V=50, dtype=np.float32, n_frames=None):
    """cases: [(emit (T, L + 1) float32, y)].  n_frames: what the kernel is told (default: each case's T).  Every output lives in
    guarded memory and is compared with the restatement in `dtype`; -> the device's statuses."""
    n = len(cases)
    E = max_tokens + 1
    emit = np.full((n, max_frames, E), np.nan, np.float32)             # what the trellis never asks for is NaN
    tok0, tokens = [0], []
    for u, (e, y) in enumerate(cases):
        if e.shape[0] <= max_frames and len(y) <= max_tokens:
            emit[u, :e.shape[0], :len(y) + 1] = e
        tokens += list(y)
        tok0.append(len(tokens))
    frames = [e.shape[0] for e, _ in cases] if n_frames is None else n_frames
    desc = ops.ctc_align_desc(n, V, blank, max_frames, max_tokens)
    nbytes = ops.ctc_align_workspace_size(desc)
    assert nbytes >= n * max_frames * (2 * max_tokens + 1)
    ws = guarded.flat_out((nbytes,), torch.uint8)
    nt = len(tokens)
    outs = (guarded.flat_out((n,), torch.float32), guarded.flat_out((n,), torch.int32), guarded.flat_out((n, max_frames), torch.int32),
            guarded.flat_out((nt,), torch.int32), guarded.flat_out((nt,), torch.int32), guarded.flat_out((nt,), torch.int32),
            guarded.flat_out((nt,), torch.float32))
    ops.ctc_align_path(desc, torch.from_numpy(emit).cuda(), _i32(frames), _i32(tokens), _i32(tok0), ws.view,
                       out=tuple(g.view for g in outs))
    torch.cuda.synchronize()
    names = ("score", "status", "state", "tok_start", "tok_end", "tok_peak", "tok_logp")
    ws.check("workspace")
    for g, name in zip(outs, names):
        g.check(name)
        assert not bool(g.untouched().any()), "%s: an element was never written" % name
    score, status, state, ts, te, tp, tl = (g.view.cpu().numpy() for g in outs)
    for u, (e, y) in enumerate(cases):
        T, L = frames[u], len(y)
        if not 0 <= T <= max_frames or L > max_tokens or any(v == blank or not 0 <= v < V for v in y):
            want = R._failed(R.BAD_INPUT, 0, L, np.float32)
        else:
            want = R.align_emit_ref(e, y, dtype)
        what = "utterance %d (T = %d, L = %d)" % (u, T, L)
        assert int(status[u]) == want.status, what
        assert np.float32(want.score).tobytes() == score[u].tobytes(), (what, score[u], want.score)
        row = np.full(max_frames, -1, np.int32)
        row[:len(want.state)] = want.state
        assert np.array_equal(state[u], row), what
        lo, hi = tok0[u], tok0[u + 1]
        assert np.array_equal(ts[lo:hi], want.start) and np.array_equal(te[lo:hi], want.end), what
        assert np.array_equal(tp[lo:hi], want.peak), what
        assert tl[lo:hi].tobytes() == want.peak_logp.astype(np.float32).tobytes(), what
    return status.tolist()


def _random_case(rng, T, L, n_sym=4, quarter=False):
    """emissions in [-8, 0) (quarter: multiples of 1/4 in [-2, 0]) and L tokens over n_sym symbols: neighbours often repeat"""
    if quarter:
        e = -(rng.integers(0, 9, size=(T, L + 1)) / 4.0)
    else:
        e = -8.0 * rng.random((T, L + 1))
    return e.astype(np.float32), [int(v) for v in rng.integers(1, 1 + n_sym, size=L)]


def test_path_small_shapes_equal_the_float32_restatement():
    """(1, 0), (1, 1), (2, 1), (7, 0); y = [a, a, b, b] at T = L + repeats (one feasible path) and one frame less (status 1);
    (70, 33): S = 67 crosses a wave.  One launch."""
    rng = np.random.default_rng(1)
    cases = [_random_case(rng, T, L) for T, L in ((1, 0), (1, 1), (2, 1), (7, 0))]
    aabb = [3, 3, 5, 5]
    cases.append((_random_case(rng, 6, 4)[0], aabb))
    cases.append((_random_case(rng, 5, 4)[0], aabb))
    cases.append(_random_case(rng, 70, 33))
    status = _run_path(cases, 70, 33)
    assert status == [0, 0, 0, 0, 0, 1, 0]
    assert R.align_emit_ref(cases[4][0], aabb).state.tolist() == [1, 2, 3, 5, 6, 7]


def test_path_more_states_than_a_work_group():
    """(1300, 600): S = 1201 > 1024 threads, every thread owns several states; a short utterance rides in the same launch"""
    rng = np.random.default_rng(2)
    cases = [_random_case(rng, 1300, 600), _random_case(rng, 9, 3)]
    assert _run_path(cases, 1300, 600) == [0, 0]


def test_path_ragged_batch_and_bad_utterances():
    """n = 5: T = 0 with L = 0 (ok, score 0), T = 0 with tokens (status 1), an utterance with more than max_tokens tokens and
    one that holds the blank (both status 2), and a healthy one in between: the neighbours' outputs are untouched"""
    rng = np.random.default_rng(3)
    e_blank, _ = _random_case(rng, 6, 2)
    cases = [(np.zeros((0, 1), np.float32), []), _random_case(rng, 12, 5), (np.zeros((0, 3), np.float32), [2, 4]),
             (_random_case(rng, 12, 7)[0], [1, 2, 3, 4, 1, 2, 3]), (e_blank, [4, 0])]
    assert _run_path(cases, 12, 5) == [0, 0, 1, 2, 2]
    # a frame count outside [0, max_frames] and a token past V: status 2 as well
    assert _run_path([_random_case(rng, 4, 2), _random_case(rng, 4, 2), (_random_case(rng, 4, 1)[0], [50])], 4, 2,
                     n_frames=[5, 4, 4]) == [2, 0, 2]


def test_path_ties_equal_the_float64_restatement():
    """emissions that are multiples of 1/4 in [-2, 0]: float32 sums are exact, ties are everywhere, and the result must be
    the float64 restatement's"""
    rng = np.random.default_rng(4)
    cases = [_random_case(rng, T, L, n_sym=2, quarter=True) for T, L in ((2, 1), (7, 0), (12, 4), (70, 33), (40, 9), (64, 31))]
    cases.append((np.zeros((9, 4), np.float32), [1, 1, 2]))            # all equal: stay over step over skip decides every cell
    status = _run_path(cases, 70, 33, dtype=np.float64)
    assert status[-1] == 0 and 0 in status[:3]
    _run_path(cases, 70, 33, dtype=np.float32)


# ---------------------------------------------------------------- 2. the emit stage against float64
@pytest.mark.parametrize("V", [2, 5, 63, 64, 65, 1434])
@pytest.mark.parametrize("odd_ld", [False, True])
def test_emit_against_float64(V, odd_ld):
    """n = 3 utterances whose rows lie out of order in a guarded, strided logits operand (ldl > V; odd_ld: rows that are only
    4-byte aligned); a tenth of the logits is -inf; L = 0 and T = 0 take part"""
    rng = np.random.default_rng(V)
    frames, row0 = [5, 0, 3], [4, 2, 0]
    toks = [[int(v) for v in rng.integers(1, V, size=6)], [1], []]
    x = (4.0 * rng.standard_normal((9, V))).astype(np.float32)
    hole = rng.random((9, V)) < 0.1
    hole[np.arange(9), rng.integers(0, V, size=9)] = False             # every row keeps a finite value
    x[hole] = -np.inf
    gx = guarded.strided_in(torch.from_numpy(x), ld=V + 7 + (2 if (V + 7) % 4 == 0 else 0) if odd_ld else None)
    assert gx.ld > V and (gx.ld % 4 != 0) == odd_ld
    max_frames, max_tokens = 5, 6
    desc = ops.ctc_align_desc(3, V, 0, max_frames, max_tokens)
    gemit = guarded.flat_out((3, max_frames, max_tokens + 1), torch.float32)
    tok0 = [0, 6, 7, 7]
    ops.ctc_align_emit(desc, gx.view, _i32(row0), _i32(frames), _i32(sum(toks, [])), _i32(tok0), emit=gemit.view)
    torch.cuda.synchronize()
    gemit.check("emit")
    got, untouched = gemit.view.cpu().numpy(), gemit.untouched().cpu().numpy()
    l64, l32 = R.log_softmax_ref(x, np.float64), R.log_softmax_ref(x, np.float32)
    err = e32 = 0.0
    for u in range(3):
        cols = [0] + toks[u]
        assert untouched[u, frames[u]:].all() and untouched[u, :, len(cols):].all()
        assert not untouched[u, :frames[u], :len(cols)].any()
        for t in range(frames[u]):
            want, w32, g = l64[row0[u] + t, cols], l32[row0[u] + t, cols], got[u, t, :len(cols)]
            inf = np.isinf(want)
            assert np.array_equal(np.isneginf(g), inf)
            if (~inf).any():
                err = max(err, float(np.abs(g[~inf] - want[~inf]).max()))
                e32 = max(e32, float(np.abs(w32[~inf].astype(np.float64) - want[~inf]).max()))
    bound = max(8 * e32, 1e-5)
    print("emit V = %d ld = %d: device err %.3e, e32 %.3e, bound %.3e" % (V, gx.ld, err, e32, bound))
    assert err <= bound, (err, bound)


# ---------------------------------------------------------------- 3. / 4. end to end on engine logits
FEAT_SEED = 1          # picked on the CPU (oracle/encoder_ref.py): the smallest top-two gap of any frame is 2.3e-2 / 4.0e-2


@pytest.fixture(scope="module")
def engine_run(golden):
    """the tiny golden model on two utterances of 90 / 61 feature frames (21 / 14 output frames): (logits on the device, output
    lengths, float64 log-probabilities per utterance, b = the emit stage's bound on these rows)"""
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg, z = golden("tiny")
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=int(z["weight_seed"])))
    feat = torch.rand(2, 90, cfg.input_dim, generator=torch.Generator().manual_seed(FEAT_SEED))
    lens = torch.tensor([[90, 61]], dtype=torch.int32)
    logits = eng(feat.cuda(), lens.cuda()).clone()
    out_lens = eng.buffer("lens", torch.int32)[:2].cpu().tolist()
    assert out_lens == [21, 14]
    x = logits.cpu().numpy()
    l64 = [R.log_softmax_ref(x[u, :n], np.float64) for u, n in enumerate(out_lens)]
    e32 = max(float(np.abs(R.log_softmax_ref(x[u, :n], np.float32).astype(np.float64) - l64[u]).max()) for u, n in enumerate(out_lens))
    b = max(8 * e32, 1e-5)
    print("engine logits: e32 %.3e, b %.3e" % (e32, b))
    return eng, logits, out_lens, l64, b


def _margin(T, b, optimum):
    return 2 * T * b + 2 * T * float(np.spacing(np.float32(abs(optimum))))


def test_aligner_end_to_end_is_optimal_within_the_margin(engine_run):
    """CtcAligner.align on engine logits for the greedy hypothesis, a damaged one (first token dropped, last one doubled) and
    a random one: a valid alignment whose float64 re-score is within 2 T b + 2 T ulp32(|optimum|) of the float64 optimum"""
    from m3asr.align import CtcAligner
    from m3asr.decode import CtcDecoder
    eng, logits, out_lens, l64, b = engine_run
    V = logits.shape[-1]
    greedy = CtcDecoder(eng).greedy_from_logits(logits, torch.tensor(out_lens, dtype=torch.int32).cuda())
    assert all(len(g) >= 3 for g in greedy)
    rng = np.random.default_rng(5)
    aligner = CtcAligner(V)
    for name, hyps in (("greedy", greedy), ("damaged", [g[1:] + g[-1:] for g in greedy]),
                       ("random", [[int(v) for v in rng.integers(1, V, size=5)] for _ in greedy])):
        got = aligner.align(logits, out_lens, hyps)
        for u, (a, y) in enumerate(zip(got, hyps)):
            T = out_lens[u]
            want = R.ctc_align_ref(l64[u], y, 0, np.float64)
            assert want.status == R.OK and a.ok and a.tokens == y
            assert len(a.states) == T and R.is_valid_path(a.states, y) and R.collapse(R.path_labels(a.states, y)) == y
            rescored = float(sum(l64[u][t, v] for t, v in enumerate(R.path_labels(a.states, y))))
            margin = _margin(T, b, float(want.score))
            print("%s utterance %d: device score %.6f, its path in float64 %.6f, float64 optimum %.6f, margin %.3e" % (
                name, u, a.score, rescored, float(want.score), margin))
            assert rescored >= float(want.score) - margin and rescored <= float(want.score) + 1e-12
            assert abs(a.score - rescored) <= margin
            for i in range(len(y)):                                    # the spans, peaks and confidences belong to that path
                span = [t for t, s in enumerate(a.states) if s == 2 * i + 1]
                assert (a.start[i], a.end[i]) == (span[0], span[-1] + 1) and a.start[i] <= a.peak[i] < a.end[i]
                assert abs(a.conf[i] - float(np.exp(l64[u][span, y[i]].max()))) <= 2 * b
                assert (a.start_ms[i], a.end_ms[i], a.peak_ms[i]) == (40 * a.start[i], 40 * a.end[i], 40 * a.peak[i])
    assert aligner.workspace is not None
    kept = aligner.workspace.data_ptr()
    aligner.align(logits, out_lens, [[1], [2]])                        # a smaller batch reuses the workspace
    assert aligner.workspace.data_ptr() == kept
    no = aligner.align(logits, [2, 14], [greedy[0], greedy[1]])[0]     # two frames cannot hold the hypothesis
    assert not no.ok and no.start == [] and no.score == NINF
    with pytest.raises(ValueError):
        aligner.align(logits, out_lens, [[0], [1]])
    same = CtcDecoder(eng).align_from_logits(logits, torch.tensor(out_lens), greedy)
    assert same == aligner.align(logits, out_lens, greedy)


def test_greedy_hypothesis_aligns_to_the_argmax_path(engine_run):
    """the Viterbi path of the greedy hypothesis is the per-frame argmax path: the score is the sum of the per-frame maxima
    within the margin, and the state matches the argmax label on every frame whose float64 top-two gap exceeds 2 b -- with
    FEAT_SEED that is every frame (asserted)"""
    from m3asr.align import CtcAligner
    from m3asr.decode import CtcDecoder
    eng, logits, out_lens, l64, b = engine_run
    greedy = CtcDecoder(eng).greedy_from_logits(logits, torch.tensor(out_lens, dtype=torch.int32).cuda())
    got = CtcAligner(logits.shape[-1]).align(logits, out_lens, greedy)
    for u, (a, y) in enumerate(zip(got, greedy)):
        T = out_lens[u]
        top = np.sort(l64[u], axis=-1)
        gap = top[:, -1] - top[:, -2]
        best = l64[u].argmax(-1)
        assert R.collapse(best.tolist()) == y
        total = float(top[:, -1].sum())
        margin = _margin(T, b, total)
        print("utterance %d: score %.6f, sum of maxima %.6f, margin %.3e, smallest top-two gap %.3e (2 b = %.3e)" % (
            u, a.score, total, margin, float(gap.min()), 2 * b))
        assert a.ok and abs(a.score - total) <= margin
        assert bool((gap > 2 * b).all()), "the seed leaves a frame of utterance %d undecided" % u
        assert R.path_labels(a.states, y) == best.tolist()


# ---------------------------------------------------------------- 5. streaming
C, MAXF, BEAM = 4, 16, 4          # as tests/test_stream_rescore_gpu.py
L_FRAMES = 10


@pytest.fixture(scope="module")
def stream_engine():
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=C, num_decoding_left_chunks=2)
    return Engine.from_state_dict(cfg, make_weights(cfg, seed=47), packed_rows=False)


def _stream_decoder(eng, B=2, **kw):
    from m3asr.align import CtcAligner
    from m3asr.decode import StreamingCtcDecoder
    return StreamingCtcDecoder(eng.streaming(B, MAXF, independent=True), beam=BEAM, aligner=CtcAligner(eng.cfg.output_dim), **kw)


def _feed(dec, b, frames, kept=None, ended=True):
    """a session in slot b, fed whole; the logits step() returned for the frames that count are appended to `kept`"""
    from m3asr.serve import WindowBuffer
    buf = WindowBuffer(C, frames.shape[1])
    buf.push(frames)
    if ended:
        buf.end()
    win = torch.zeros(dec.beam.B, 4 * C + 3, frames.shape[1])
    while buf.ready() > 0:
        valid = torch.zeros(dec.beam.B, dtype=torch.int32)
        _, valid[b] = buf.take(out=win[b])
        n = int(dec.frames_of(valid)[b])
        logits = dec.step(win, valid)
        dec.st.eng.stream.synchronize()
        if kept is not None:
            kept.append(logits[b, :n].clone())


def test_streaming_align_equals_offline_alignment_of_the_kept_logits(stream_engine):
    """slot 1 runs a session that is reset mid-way; slot 0's alignment must equal, exactly, the offline alignment of the
    logits step() returned for it (the same kernels on the same bits), for its own best hypothesis and for a given one"""
    from m3asr.align import CtcAligner
    eng = stream_engine
    V = eng.cfg.output_dim
    g = torch.Generator().manual_seed(3)
    feats = [torch.rand(45, eng.cfg.input_dim, generator=g), torch.rand(35, eng.cfg.input_dim, generator=g)]
    dec = _stream_decoder(eng)
    kept = {0: [], 1: []}
    _feed(dec, 1, feats[0][:4 * C + 3])                                # a first occupant of slot 1: one chunk
    _feed(dec, 0, feats[0][:4 * C * 2 + 3], kept[0], ended=False)      # slot 0: two chunks ...
    dec.reset(slots=[1])                                               # ... the other slot is restarted mid-way ...
    _feed(dec, 1, feats[1], kept[1])                                   # ... and slot 0 goes on with its last, short window
    rest = feats[0][4 * C * 2:]
    valid = torch.zeros(2, dtype=torch.int32)
    win = torch.zeros(2, 4 * C + 3, eng.cfg.input_dim)
    win[0, :rest.shape[0]] = rest
    valid[0] = rest.shape[0]
    n = int(dec.frames_of(valid)[0])
    logits = dec.step(win, valid)
    eng.stream.synchronize()
    kept[0].append(logits[0, :n].clone())
    rows = {b: torch.cat(kept[b]) for b in kept}
    assert [rows[0].shape[0], rows[1].shape[0]] == [10, 8]
    best = [list(h[0][0]) for h in dec.finish()]
    offline = CtcAligner(V)
    for b in (0, 1):
        want, = offline.align_rows(rows[b], [0], [rows[b].shape[0]], [best[b]])
        got, = dec.align(slots=[b])
        assert got == want and got.ok == (want.score > NINF), b
        if best[b]:
            other = best[b][:-1]
            assert dec.align(slots=[b], tokens=[other]) == offline.align_rows(rows[b], [0], [rows[b].shape[0]], [other])
    both = dec.align()
    assert both == [dec.align(slots=[0])[0], dec.align(slots=[1])[0]] and dec.align(slots=[]) == []
    assert [list(h[0][0]) for h in dec.finish()] == best             # the streams go on as they were
    with pytest.raises(ValueError):
        dec.align(slots=[0], tokens=[[0]])


def test_streaming_align_past_max_frames_and_without_an_aligner(stream_engine):
    from m3asr.decode import StreamingCtcDecoder
    eng = stream_engine
    dec = _stream_decoder(eng)
    g = torch.Generator().manual_seed(4)
    _feed(dec, 1, torch.rand(4 * C + 3, eng.cfg.input_dim, generator=g))
    _feed(dec, 0, torch.rand(4 * C * 4 + 3, eng.cfg.input_dim, generator=g), ended=False)     # four chunks fill the slot: MAXF frames
    assert len(dec.align(slots=[0])[0].states) == MAXF
    # a fifth chunk: a host `valid` is refused before the launch, so the frame counts go as device data and the guards are the
    # kernels' own (tests/test_stream_slots_gpu.py): the searches and the store mark the slot, nothing is consumed
    win = torch.rand(2, 4 * C + 3, eng.cfg.input_dim, generator=g)
    dec.step(win, torch.tensor([4 * C + 3, 0], dtype=torch.int32).cuda())
    got = dec.align()
    assert got[0] is None and got[1] is not None and len(got[1].states) == C
    assert dec.align(slots=[0], tokens=[[1]]) == [None]
    dec.reset(slots=[0])                                               # the store is cleared with the rest
    assert dec.align(slots=[0]) != [None]
    plain = StreamingCtcDecoder(eng.streaming(2, MAXF, independent=True), beam=BEAM)
    assert plain.aligner is None and not hasattr(plain, "lstate") and not hasattr(plain, "lrows")
    with pytest.raises(M3Error, match="aligner"):
        plain.align()
    assert plain.beam.state.numel() == dec.beam.state.numel() == ops.ctc_beam_state_size(plain.beam.desc)
    assert plain.gstate.numel() == dec.gstate.numel() == ops.ctc_greedy_stream_state_size(plain.gdesc)
    from m3asr.align import CtcAligner
    with pytest.raises(M3Error, match="aligner"):
        StreamingCtcDecoder(eng.streaming(2, MAXF, independent=True), beam=BEAM, aligner=CtcAligner(eng.cfg.output_dim - 1))


def test_pool_files_timed_segments_in_session_time(stream_engine):
    """the length rule of tests/test_stream_rescore_gpu.py (fires in a slot's third chunk): every segment's times equal those
    of a fresh session fed that segment's frames, moved by the chunks before it -- 12 frames per earlier segment"""
    from m3asr.align import token_times
    from m3asr.decode import EndpointConfig
    from m3asr.serve import StreamPool, TimedSegment
    eng = stream_engine
    rule = EndpointConfig(rules=((False, 0, L_FRAMES * 40),))
    per_seg = -(-L_FRAMES // C)
    feat = torch.rand(4 * C * 13 + 3, eng.cfg.input_dim, generator=torch.Generator().manual_seed(21))
    pool = StreamPool(_stream_decoder(eng, endpoint=rule), segment=True, timestamps=True)
    sid = pool.open()
    pool.push(sid, feat)
    segs = []
    while pool.step():
        segs += pool.segments(sid)
    ref = _stream_decoder(eng, endpoint=rule)
    seen = 0
    for j in range(4):
        f0 = 4 * C * per_seg * j
        ref.reset(slots=[0])
        _feed(ref, 0, feat[f0:f0 + 4 * C * per_seg + 3], ended=False)
        nbest = ref.finish(slots=[0])[0]
        if not nbest or len(nbest[0][0]) == 0:
            continue
        seg = segs[seen]
        seen += 1
        assert isinstance(seg, TimedSegment) and seg.nbest == nbest and seg.end_frame == per_seg * C * j + L_FRAMES - 1
        a, = ref.align(slots=[0])
        assert a.ok and seg.times == token_times(a, 40, per_seg * C * j)
        assert [t[0] for t in seg.times] == list(nbest[0][0])
        assert all(per_seg * C * j * 40 <= t[1] < t[2] <= per_seg * C * (j + 1) * 40 for t in seg.times)
        print("segment %d: %s" % (j, seg.times))
    assert seen == len(segs) and seen >= 2, "the random model decodes nothing: the comparison would be empty"
    assert any(t[1] >= per_seg * C * 40 for s in segs[1:] for t in s.times)
    off = pool.offset_ms(sid)
    rest, times = pool.close(sid, timed=True)
    assert off == 4 * per_seg * C * 40 and (times is None or all(t[1] >= off for t in times))


# ---------------------------------------------------------------- 6. the command lines
def _cli(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def built_plan(tmp_path_factory):
    """synthetic CTC/attention checkpoint -> builder.py -> (directory, plan, feat.npy, words.txt, lm.arpa)"""
    import lm_ref
    d = str(tmp_path_factory.mktemp("align_cli"))
    _cli(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--decoder-blocks", "2", "--seed", "4"])
    plan = os.path.join(d, "aed.plan")
    _cli(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", os.path.join(d, "model.pt"), "-o", plan, "--opt-shape", "2x80"])
    feat = os.path.join(d, "feat.npy")
    np.save(feat, torch.rand(2, 90, 40, generator=torch.Generator().manual_seed(7)).numpy())
    from m3asr.plan import load_plan
    V = load_plan(plan)[0].output_dim
    words = os.path.join(d, "words.txt")
    with open(words, "w") as f:
        f.write("1 2\n3\n")
    arpa = os.path.join(d, "lm.arpa")
    with open(arpa, "w", encoding="utf-8") as f:
        f.write(lm_ref.random_arpa(np.random.default_rng(5), V, 3, min(12, V - 1), 40)[1])
    return plan, feat, words, arpa, V


@pytest.mark.parametrize("family", ["plain", "hotwords", "lm", "rescore", "attention"])
def test_infer_timestamps_command_line(built_plan, family):
    """infer.py --timestamps in a child process, one decoding family per case: a `times` block per utterance whose lines
    parse, with times that do not decrease, lie inside the utterance and are multiples of 40 ms; and the same command without
    the flag prints that output without the blocks (the wall-clock lines aside) -- what it printed before there was a flag"""
    plan, feat, words, arpa, V = built_plan
    extra = {"plain": ("greedy", []), "hotwords": ("biased", ["--hotwords", words, "--beam", "4"]),
             "lm": ("fused", ["--lm", arpa, "--beam", "4"]), "rescore": ("rescored", ["--rescore", "--beam", "4", "--ctc-weight", "0.3"]),
             "attention": ("attention", ["--attention", "--beam", "3", "--max-steps", "6"])}
    mode, flags = extra[family]
    cmd = ["infer.py", "-p", plan, "-i", feat] + flags
    timed, plain = _cli(cmd + ["--timestamps"]).splitlines(), _cli(cmd).splitlines()
    clock = lambda lines: [l for l in lines if not l.startswith("time=")]
    first = timed.index("utt 0 %s times:" % mode)
    assert clock(timed[:first]) == clock(plain) and not any("times:" in l for l in plain)
    blocks, cur = {}, None
    for line in timed[first:]:
        m = re.match(r"^utt (\d+) %s times:$" % mode, line)
        if m:
            cur = blocks.setdefault(int(m.group(1)), [])
        else:
            cur.append(line)
    assert sorted(blocks) == [0, 1]
    frames = 21                                                        # 90 feature frames
    n_tokens = 0
    for u, lines in blocks.items():
        if lines == ["no alignment"]:
            continue
        last = 0
        for line in lines:
            m = re.match(r"^(\d+) (\d+) (\d+) ([01]\.\d{4})$", line)
            assert m, line
            tok, t0, t1, conf = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4))
            assert 1 <= tok < V and t0 % 40 == 0 and t1 % 40 == 0 and last <= t0 < t1 <= frames * 40 and 0.0 <= conf <= 1.0
            last = t1
            n_tokens += 1
    print("%s: %d token lines" % (family, n_tokens))
    if family in ("plain", "hotwords", "lm", "rescore"):               # hypotheses CTC itself produced always align
        assert n_tokens > 0 and all(lines != ["no alignment"] for lines in blocks.values())


def test_transcribe_stream_timestamps_command_line():
    """--synthetic 3 --timestamps, cut every second by a length rule: the token lines behind a segment line lie inside the
    session, do not decrease, and carry the segment's tokens"""
    out = _cli(["tools/transcribe_stream.py", "--synthetic", "3", "--timestamps", "--beam", "4", "--rule", "0,0,1000"])
    segs, cur = [], None
    for line in out.splitlines():
        m = re.match(r"^(\d+)-(\d*) ms rule (\d+): ([\d ]*)$", line)
        if m:
            cur = ([int(t) for t in m.group(4).split()], [])
            segs.append(cur)
            continue
        m = re.match(r"^(\d+) (\d+) (\d+) ([01]\.\d{4})$", line)
        if m and cur is not None:
            cur[1].append((int(m.group(1)), int(m.group(2)), int(m.group(3))))
    assert len(segs) >= 2 and any(times for _, times in segs)
    last = 0
    for tokens, times in segs:
        assert [t[0] for t in times] == tokens
        for _, t0, t1 in times:
            assert t0 % 40 == 0 and last <= t0 < t1 <= 3000 + 40
            last = t1
