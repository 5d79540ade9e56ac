"""The long-form path on the device (csrc/vad.hip, m3asr.frontend.EnergyVad / segment_gather, m3asr.longform)
against the float64 restatement of its contracts (tests/vad_ref.py).  Every device output is a guarded operand
(tests/guarded.py): a store past a row, a column or `capacity` is caught.

Bounds.  Log-energy: E is a sum of 400 squares of (x - mean); about 404 fp32 roundings of 2^-24 each give a relative error on
E of at most 2.4e-5, which is the absolute error of log E; the mean's own error enters in second order only (sum (x - m)^2 is
stationary at the true mean).  The bound 1e-4 has 4x headroom on top.  The signals have |mean| <= rms and E >= 1, so neither
cancellation nor the floor is in play; the floor has a row of its own.  Flags, segment lists, counts and gathered rows are
exact.  For the flags that needs every log-energy to be clear of the threshold: the test asserts a margin of 1e-3 on the CPU
first (the threshold itself is one float64 expression rounded once on both sides; only the order of the mean's float64 sum
differs, by parts in 1e16)."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G
import vad_cases
import vad_ref as R
from m3asr import _lib
from m3asr.frontend import EnergyVad, VadConfig, segment_gather

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(zip(("min_silence", "min_speech", "pad", "max_segment", "split_search"), vad_cases.OPTS))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------- (a) log-energy

def _signals():
    """rows of 399, 400 and 400 + 160 * 37 + 159 samples: noise of rms ~ 1000 around a DC offset of 300, and a row of equal
    samples"""
    rng = np.random.default_rng(5)
    lens = [399, 400, 400 + 160 * 37 + 159]
    N = lens[-1]
    x = np.zeros((4, N), dtype=np.int16)
    for b, n in enumerate(lens):
        x[b, :n] = np.clip(np.round(rng.normal(300, 1000, n)), -32768, 32767).astype(np.int16)
    x[3] = 1234
    return x, lens + [N]


def test_log_energy():
    x, lens = _signals()
    B, N = x.shape
    T = R.num_frames(N) + 1                                        # one more than the longest row needs
    vad = EnergyVad(VadConfig(), "cuda:0")
    got = {}
    for name, pcm in (("int16", torch.from_numpy(x)), ("float32", torch.from_numpy(x).float())):
        out, out_len = G.strided_out(B, T), G.flat_out((B,), torch.int32)
        vad.log_energy(pcm, torch.tensor(lens), out=out.view, out_len=out_len.view)
        torch.cuda.synchronize()
        out.check("logE (%s)" % name)
        out_len.check("len_out (%s)" % name)
        assert out_len.view.cpu().tolist() == [0, 1, 38, 38]
        got[name] = out.view.cpu()
    assert G.same_bits(got["int16"], got["float32"]), "int16 and float32 input give the same bits"
    g = got["int16"].numpy()
    worst = 0.0
    for b in range(3):
        want, n = R.log_energy(x[b, :lens[b]], T)
        sig = x[b, :lens[b]].astype(np.float64)
        for k in range(n):                                         # the test's own preconditions
            f = sig[160 * k: 160 * k + 400]
            assert abs(f.mean()) <= np.sqrt((f ** 2).mean()) and ((f - f.mean()) ** 2).sum() >= 1.0
        err = np.abs(g[b, :n].astype(np.float64) - want[:n])
        worst = max(worst, float(err.max()) if n else 0.0)
        assert not g[b, n:].any(), "row %d: frames behind the last are zeros" % b
        assert np.all(err <= 1e-4), "row %d: |delta| %.3e" % (b, float(err.max()))
    print("log-energy: worst |delta| %.3e (bound 1e-4)" % worst)
    floor = np.float32(np.log(np.float64(np.finfo(np.float32).eps)))
    assert np.all(g[3, :38] == floor) and g[3, 38] == 0.0, "equal samples: the floor log(FLT_EPSILON)"


def test_log_energy_refusals_and_empty():
    lib = _lib.load()
    pcm = torch.zeros(1, 808, dtype=torch.int16, device="cuda")
    n, out, ln = _i32([808]), torch.full((1, 3), -7.0, device="cuda"), _i32([-1])

    def call(ld_pcm=808, T=3, ld_out=3, B=1, ptr=None):
        return lib.m3_vad_log_energy(pcm.data_ptr() if ptr is None else ptr, 1, ld_pcm, n.data_ptr(), B, T, out.data_ptr(), ld_out,
                                     ln.data_ptr(), None)

    for kw, msg in ((dict(ld_pcm=804), "ld_pcm=804"), (dict(ld_out=2), "ld_out=2"), (dict(ptr=pcm.data_ptr() + 2), "aligned"),
                    (dict(B=-1), "bad sizes")):
        assert call(**kw) != 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(B=0) == 0 and call(T=0) == 0
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and ln.item() == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert ln.item() == 3 and out[0].cpu().tolist() == [float(np.float32(np.log(np.float64(np.finfo(np.float32).eps))))] * 3


# ---------------------------------------------------------------- (b) decide

DECIDE_LENS = [1, 2, 64, 65, 257]                                  # across a wave and a 256-lane group


def _decide_inputs():
    """log-energies fed in directly (both sides see the same bits); garbage behind every row's length"""
    rng = np.random.default_rng(11)
    T = max(DECIDE_LENS) + 1
    e = np.full((len(DECIDE_LENS), T), 1e9, dtype=np.float32)
    for b, n in enumerate(DECIDE_LENS):
        e[b, :n] = rng.normal(8.0, 4.0, n).astype(np.float32)
    return e


@pytest.mark.parametrize("mean_scale", [0.0, 0.5])
@pytest.mark.parametrize("context", [0, 2])
def test_decide(context, mean_scale):
    e = _decide_inputs()
    B, T = e.shape
    for b, n in enumerate(DECIDE_LENS):                            # on the CPU, before anything runs: no frame near the threshold
        assert R.margin(e[b], n, 5.0, mean_scale) >= 1e-3, "row %d: a log-energy within 1e-3 of the threshold" % b
    vad = EnergyVad(VadConfig(energy_mean_scale=mean_scale, context=context), "cuda:0")
    logE = G.strided_in(torch.from_numpy(e))
    flags, thr = G.strided_out(B, T, torch.uint8), G.flat_out((B,), torch.float32)
    vad.decide(logE.view, _i32(DECIDE_LENS), flags=flags.view, threshold=thr.view)
    torch.cuda.synchronize()
    flags.check("flags")
    thr.check("threshold")
    got, got_thr = flags.view.cpu().numpy(), thr.view.cpu().numpy()
    for b, n in enumerate(DECIDE_LENS):
        want, want_thr = R.decide(e[b], n, 5.0, mean_scale, context, 0.6)
        assert abs(float(got_thr[b]) - float(want_thr)) <= 2e-6 * max(1.0, abs(float(want_thr)))
        assert np.array_equal(got[b], want), "row %d (len %d)" % (b, n)
        assert 0 < want[:n].sum() < n or n <= 2


def test_decide_across_tiles_and_refusals():
    """a row longer than one work-group's tile of 4096 frames, with the widest context; bad options"""
    rng = np.random.default_rng(12)
    n, T = 9000, 9001
    e = rng.choice(np.array([2.0, 3.0, 12.0, 14.0], dtype=np.float32), size=(1, T))
    assert R.margin(e[0], n, 5.0, 0.25) >= 1e-3
    vad = EnergyVad(VadConfig(energy_mean_scale=0.25, context=32, proportion_threshold=0.45), "cuda:0")
    flags = G.strided_out(1, T, torch.uint8)
    vad.decide(torch.from_numpy(e).cuda(), _i32([n]), flags=flags.view)
    torch.cuda.synchronize()
    flags.check("flags")
    want, _ = R.decide(e[0], n, 5.0, 0.25, 32, 0.45)
    assert np.array_equal(flags.view.cpu().numpy()[0], want) and 0 < want.sum() < n
    lib = _lib.load()
    x, ln, f, t = torch.zeros(1, 8, device="cuda"), _i32([8]), torch.zeros(1, 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, device="cuda")

    def call(scale=0.5, context=0, prop=0.6, ld=8):
        return lib.m3_vad_decide(x.data_ptr(), ld, ln.data_ptr(), 1, 8, 5.0, scale, context, prop, f.data_ptr(), 8, t.data_ptr(), None)

    assert call() == 0
    for kw, msg in ((dict(context=33), "context=33"), (dict(context=-1), "context=-1"), (dict(prop=0.0), "proportion"),
                    (dict(prop=1.0), "proportion"), (dict(scale=-1.0), "energy_mean_scale"), (dict(ld=7), "shorter")):
        assert call(**kw) != 0 and msg in _lib.last_error(), (kw, _lib.last_error())


# ---------------------------------------------------------------- (c) segments

def _run_segments(flags, logE, lens, capacity, cfg):
    """one launch on guarded outputs -> (lists of the written entries, counts, the guarded segment buffer)"""
    B = flags.shape[0]
    vad = EnergyVad(cfg, "cuda:0")
    seg, cnt = G.flat_out((B, capacity, 2), torch.int32), G.flat_out((B,), torch.int32)
    vad.segments(G.strided_in(torch.from_numpy(flags), int_guard=1).view, G.strided_in(torch.from_numpy(logE)).view, _i32(lens),
                 capacity, segments=seg.view, n_segments=cnt.view)
    torch.cuda.synchronize()
    seg.check("segments")
    cnt.check("n_segments")
    counts = cnt.view.cpu().tolist()
    rows = seg.view.cpu()
    untouched = seg.untouched().cpu()
    lists = []
    for b in range(B):
        k = min(counts[b], capacity)
        assert not untouched[b, :k].any() and untouched[b, k:].all(), "row %d: exactly the first %d entries are written" % (b, k)
        lists.append([tuple(p) for p in rows[b, :k].tolist()])
    return lists, counts


def test_segments_hand_made():
    cases = vad_cases.cases()
    T = max(len(c[1]) for c in cases)
    flags, logE = np.ones((len(cases), T), dtype=np.uint8), np.zeros((len(cases), T), dtype=np.float32)      # voiced behind a row's own frames
    for b, (_, f, e, _, _) in enumerate(cases):
        flags[b, :len(f)], logE[b, :len(e)] = f, e
    lists, counts = _run_segments(flags, logE, [c[3] for c in cases], 4, VadConfig(**SMALL))
    for b, (name, _, _, _, want) in enumerate(cases):
        assert lists[b] == want and counts[b] == len(want), name


def _random_patterns(seed, B, T):
    """flags as alternating runs of geometric length around the options' sizes, log-energies from four values: every rule
    fires often and ties occur"""
    rng = np.random.default_rng(seed)
    flags = np.zeros((B, T), dtype=np.uint8)
    lens = rng.integers(0, T + 1, B)
    lens[:3] = [T, 0, 1][:B]
    for b in range(B):
        t, on = 0, bool(rng.integers(0, 2))
        while t < T:
            n = int(rng.geometric(1.0 / rng.choice([2, 6, 12, 60] if on else [2, 5, 6, 9])))
            flags[b, t:t + n] = on
            t, on = t + n, not on
    return flags, rng.integers(0, 4, (B, T)).astype(np.float32), [int(v) for v in lens]


def test_segments_random():
    flags, logE, lens = _random_patterns(21, 200, 600)
    want = [R.segments(flags[b], logE[b], lens[b], *vad_cases.OPTS) for b in range(200)]
    assert max(len(w) for w in want) <= 64 and sum(len(w) for w in want) > 1500
    assert sum(1 for w in want for s, e in w if e - s > 36) > 50, "the split rule fires"
    lists, counts = _run_segments(flags, logE, lens, 64, VadConfig(**SMALL))
    assert counts == [len(w) for w in want]
    for b in range(200):
        assert lists[b] == want[b], "row %d (len %d)" % (b, lens[b])
    # a capacity below the count: the count is true, the first `capacity` entries are right, nothing behind them is written
    lists, counts = _run_segments(flags, logE, lens, 3, VadConfig(**SMALL))
    assert counts == [len(w) for w in want] and max(counts) > 3
    for b in range(200):
        assert lists[b] == want[b][:3], "row %d" % b
    lists, counts = _run_segments(flags[:4], logE[:4], lens[:4], 0, VadConfig(**SMALL))
    assert counts == [len(w) for w in want[:4]] and lists == [[], [], [], []]


@pytest.mark.parametrize("opts", [vad_cases.OPTS, (30, 20, 10, 3000, 500)], ids=["small", "defaults"])
def test_segments_long_row(opts):
    """one row of 70 000 frames (and a short neighbour): no single-work-group assumption.  Under the default options the runs
    are long, so the arg-min of a split walks a window of 500 frames."""
    T = 70000
    flags, logE, _ = _random_patterns(22, 2, T)
    if opts[3] == 3000:                                            # long voiced stretches: bridge most pauses
        flags[0, 5000:30000] = 1
        flags[0, 40000:47000] = 1
    lens = [T, 777]
    want = [R.segments(flags[b], logE[b], lens[b], *opts) for b in range(2)]
    assert len(want[0]) > (1000 if opts[3] == 40 else 10)
    cfg = VadConfig(**dict(zip(("min_silence", "min_speech", "pad", "max_segment", "split_search"), opts)))
    lists, counts = _run_segments(flags, logE, lens, len(want[0]) + 1, cfg)
    assert counts == [len(w) for w in want] and lists == want


def test_segments_refusals():
    lib = _lib.load()
    f, e, ln = torch.zeros(1, 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, 8, device="cuda"), _i32([8])
    seg, cnt = torch.zeros(1, 2, 2, dtype=torch.int32, device="cuda"), _i32([-1])

    def call(o=(30, 20, 10, 3000, 500), capacity=2, B=1):
        return lib.m3_vad_segments(f.data_ptr(), 8, e.data_ptr(), 8, ln.data_ptr(), B, 8, *o, seg.data_ptr(), capacity, cnt.data_ptr(), None)

    assert call() == 0
    for o, msg in (((30, 6, 10, 3000, 500), "min_speech=6"), ((19, 20, 10, 3000, 500), "exceeds min_silence"),
                   ((30, 20, 10, 3000, 2994), "split_search=2994"), ((30, 20, 10, 3000, 0), "split_search=0"),
                   ((-1, 20, 0, 3000, 500), "negative")):
        assert call(o) != 0 and msg in _lib.last_error(), (o, _lib.last_error())
    assert call(capacity=-1) != 0
    cnt.fill_(-1)
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert cnt.item() == -1


# ---------------------------------------------------------------- (d) gather

@pytest.mark.parametrize("ld_dst", [44, 45], ids=["16-byte", "scalar"])
@pytest.mark.parametrize("T_max", [101, 50])
def test_gather(T_max, ld_dst):
    """jobs of 7, 64 and 101 frames from a (300, 40) source with ld_src = 48; ld_dst = 44 takes the 16-byte path, 45 the scalar"""
    cols, B = 40, 3
    src = torch.randn(300, cols, generator=torch.Generator().manual_seed(4))
    jobs = [(0, 5, 12), (100, 20, 84), (0, 199, 300)]             # the last one ends with the matrix
    s = G.strided_in(src, ld=48)
    d = G.strided_out(B * T_max, cols, ld=ld_dst)
    ln = G.flat_out((B,), torch.int32)
    assert (s.view.data_ptr() % 16, d.view.data_ptr() % 16, s.ld, d.ld) == (0, 0, 48, ld_dst)
    dst = d.view.unflatten(0, (B, T_max))
    segment_gather(s.view, _i32(jobs), dst, ln.view, cols=cols)
    torch.cuda.synchronize()
    d.check("dst")                                                 # columns >= cols and the rows around are not touched
    ln.check("len_out")
    want = torch.zeros(B, T_max, cols)
    want_len = R.gather(src.numpy(), jobs, T_max, want.numpy())
    assert ln.view.cpu().tolist() == want_len == [min(n, T_max) for n in (7, 64, 101)]
    assert G.same_bits(dst.cpu(), want), "bit-equal to indexing; zeros in the padding frames"
    for b, (r, a, e) in enumerate(jobs):                           # ... and to torch indexing itself
        n = min(e - a, T_max)
        assert torch.equal(dst[b, :n].cpu(), src[r + a:r + a + n]) and not dst[b, n:].any()


def test_gather_refusals_and_jobs_that_leave_the_matrix():
    lib = _lib.load()
    src = torch.arange(80, dtype=torch.float32, device="cuda").view(10, 8)
    dst = torch.full((4, 6, 8), -3.0, device="cuda")
    ln = _i32([-1] * 4)
    jobs = _i32([(0, 8, 14), (0, -2, 3), (0, 12, 15), (0, 5, 2)])  # runs off the end; starts outside (twice); end < start
    segment_gather(src, jobs, dst, ln)
    torch.cuda.synchronize()
    assert ln.cpu().tolist() == [2, 0, 0, 0]
    assert torch.equal(dst[0, :2], src[8:10]) and not dst[0, 2:].any() and not dst[1:].any()

    def call(cols=8, ld_src=8, ld_dst=8, B=4):
        return lib.m3_segment_gather(src.data_ptr(), ld_src, 10, jobs.data_ptr(), B, 6, cols, dst.data_ptr(), ld_dst, 48, ln.data_ptr(), None)

    for kw, msg in ((dict(cols=0), "cols=0"), (dict(ld_src=7), "shorter"), (dict(ld_dst=7), "shorter"), (dict(B=-1), "bad sizes")):
        assert call(**kw) != 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    dst.fill_(-3.0)
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert torch.all(dst == -3.0)


# ---------------------------------------------------------------- end to end

E2E_VAD = dict(max_segment=150, split_search=60)                   # the long bursts are split


def _recording():
    """about 12 s: noise bursts of differing lengths (rms 3000) between near-silence (rms 2), int16, fixed seed"""
    rng = np.random.default_rng(31)
    x = rng.normal(0, 2, 192000)
    for start, dur in ((0.4, 0.5), (1.6, 1.3), (3.8, 2.2), (6.9, 0.9), (8.6, 3.1)):
        a, n = int(16000 * start), int(16000 * dur)
        x[a:a + n] = rng.normal(0, 3000, n)
    return torch.from_numpy(np.clip(np.round(x), -32768, 32767).astype(np.int16))


@pytest.fixture(scope="module")
def tiny():
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.longform import LongFormTranscriber
    from m3asr.weights import make_weights
    cfg = EncoderConfig.tiny()
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=3))
    lf = LongFormTranscriber(eng, vad=VadConfig(**E2E_VAD), max_batch=3, bucket=50)
    return cfg, eng, lf, _recording()


def test_e2e_segments_equal_the_restatement(tiny):
    _, eng, lf, pcm = tiny
    segs, feat = lf.segment(pcm)
    lists, logE, lens = lf.vad(pcm, detail=True)
    assert lists == [segs] and tuple(feat.shape) == (R.num_frames(192000), 40) and lens.cpu().tolist() == [feat.shape[0]]
    e = logE.cpu().numpy()[0]
    c = lf.vad_cfg
    assert R.margin(e, len(e), c.energy_threshold, c.energy_mean_scale) >= 1e-3
    flags, _ = R.decide(e, len(e), c.energy_threshold, c.energy_mean_scale, c.context, c.proportion_threshold)
    want = R.segments(flags, e, len(e), *c.segment_options())
    assert segs == want and len(segs) >= 7 and max(e - s for s, e in segs) <= 150
    assert any(a[1] == b[0] for a, b in zip(segs[:-1], segs[1:])), "a burst was split"
    # a capacity below the count: one retry with the reported count
    assert lf.vad(pcm, capacity=2) == [segs]
    # the features are those of the front end over the whole recording
    assert torch.equal(feat, lf.frontend(pcm)[0][0])


@pytest.mark.parametrize("delta_order", [0, 2])
def test_features_in_pieces_are_the_same_bits(tiny, delta_order):
    """a recording too long for one m3_fbank launch is featurised in pieces (here: of 100 and of 1 frame), deltas over the whole"""
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.longform import LongFormTranscriber
    from m3asr.weights import make_weights
    cfg, eng, lf, pcm = tiny
    if delta_order:
        cfg = EncoderConfig.tiny(input_dim=48, delta_order=2)
        lf = LongFormTranscriber(Engine.from_state_dict(cfg, make_weights(cfg, seed=3)), vad=VadConfig(**E2E_VAD))
    x = pcm[:16000 * 3 + 77]
    whole = lf.features(x).clone()
    whole8 = lf.features(x[::2], sample_rate=8000).clone()          # through the resampler's float32 staging tensor
    assert tuple(whole.shape) == tuple(whole8.shape) == (R.num_frames(x.numel()), cfg.input_dim) and torch.equal(whole, lf.frontend(x)[0][0])
    try:
        for piece in (100, 1):
            lf.piece_frames = piece
            assert torch.equal(lf.features(x), whole), "pieces of %d" % piece
            assert torch.equal(lf.features(x[::2], sample_rate=8000), whole8), "8 kHz, pieces of %d" % piece
    finally:
        lf.piece_frames = 1 << 25


def test_e2e_batches_equal_the_engine_on_the_same_batch(tiny):
    cfg, eng, lf, pcm = tiny
    ref = eng.clone_context()
    segs, feat = lf.segment(pcm)
    seen, shapes = [], set()
    for idx, logits, out_lens in lf.batches(pcm):
        B, T = len(idx), -(-max(segs[i][1] - segs[i][0] for i in idx) // 50) * 50
        batch = torch.zeros(B, T, cfg.input_dim, device="cuda")
        for b, i in enumerate(idx):
            batch[b, :segs[i][1] - segs[i][0]] = feat[segs[i][0]:segs[i][1]]
        lens = torch.tensor([segs[i][1] - segs[i][0] for i in idx], dtype=torch.int32)
        want = ref.infer(batch, lens)
        assert tuple(logits.shape) == tuple(want.shape) and torch.equal(logits, want), "batch %s" % (idx,)
        from m3asr.config import subsampled_len
        assert out_lens.cpu().tolist() == [subsampled_len(int(n)) for n in lens]
        seen += idx
        shapes.add((B, T))
    assert sorted(seen) == list(range(len(segs))) and len(shapes) >= 2 and max(b for b, _ in shapes) == 3


def test_e2e_transcribe(tiny):
    _, eng, lf, pcm = tiny
    out = lf.transcribe(pcm, mode="greedy", timestamps=True)
    segs, _ = lf.segment(pcm)
    assert [(s.start_ms, s.end_ms) for s in out] == [(10 * a, 10 * b) for a, b in segs]
    assert all(a.end_ms <= b.start_ms for a, b in zip(out[:-1], out[1:])), "time order"
    assert sum(len(s.tokens) for s in out) > 0
    for s in out:
        assert s.times is not None and [t[0] for t in s.times] == s.tokens
        for tok, a, b, conf in s.times:
            assert s.start_ms <= a < b <= s.end_ms and 0.0 < conf <= 1.0
    # a decode function of the caller's; the prefix beam search on the same batches
    mine = lf.transcribe(pcm, decode=lambda logits, lens, hidden: lf._decoder.greedy_from_logits(logits, lens))
    assert [s.tokens for s in mine] == [s.tokens for s in out] and all(s.times is None for s in mine)
    beam = lf.transcribe(pcm, mode="beam", beam_size=4)
    assert len(beam) == len(out) and all(isinstance(s.tokens, list) for s in beam)
    with pytest.raises(ValueError, match="mode"):
        lf.transcribe(pcm, mode="nope")


def test_e2e_rescore_and_attention_modes(tiny):
    """mode="rescore" / "attention" with an AED decoder: per batch what CtcDecoder's *_from_logits entry points give on another
    context of the engine fed the same batch (their hidden states come from the engine's last forward)"""
    from m3asr.config import DecoderConfig
    from m3asr.decode import CtcDecoder
    from m3asr.longform import LongFormTranscriber
    from m3asr.plan import pack_decoder
    from m3asr.rescore import AttentionRescorer
    from m3asr.weights import make_decoder_weights
    cfg, eng, lf, pcm = tiny
    dcfg = DecoderConfig.tiny()
    g = torch.Generator().manual_seed(2)
    sd = make_decoder_weights(dcfg, seed=11)
    sd["after_norm.weight"] = torch.rand(dcfg.dim, generator=g) + 0.5
    sd["after_norm.bias"] = torch.randn(dcfg.dim, generator=g) * 0.1
    rescorer = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    lf2 = LongFormTranscriber(eng.clone_context(), vad=VadConfig(**E2E_VAD), max_batch=3, bucket=50, rescorer=rescorer)
    ref = eng.clone_context()
    dec = CtcDecoder(ref, rescorer=rescorer)
    segs, feat = lf2.segment(pcm)
    want_r, want_a = [None] * len(segs), [None] * len(segs)
    for idx, T in lf2.plan_batches(segs):
        batch = torch.zeros(len(idx), T, cfg.input_dim, device="cuda")
        for b, i in enumerate(idx):
            batch[b, :segs[i][1] - segs[i][0]] = feat[segs[i][0]:segs[i][1]]
        logits = ref.infer(batch, torch.tensor([segs[i][1] - segs[i][0] for i in idx], dtype=torch.int32))
        lens = ref.buffer("lens", torch.int32)[:len(idx)].clone()
        for b, (r, a) in enumerate(zip(dec.rescore_from_logits(logits, lens, 4, ctc_weight=0.3),
                                       dec.attention_from_logits(logits, lens, 3, max_steps=6))):
            want_r[idx[b]], want_a[idx[b]] = r, a
    got_r = lf2.transcribe(pcm, mode="rescore", beam_size=4, ctc_weight=0.3)
    got_a = lf2.transcribe(pcm, mode="attention", beam_size=3, max_steps=6)
    assert [s.tokens for s in got_r] == want_r and [s.tokens for s in got_a] == want_a
    assert sum(len(t) for t in want_r) > 0 and sum(len(t) for t in want_a) > 0
    with pytest.raises(_lib.M3Error, match="rescorer"):
        lf.transcribe(pcm, mode="rescore")


def test_e2e_other_rate_and_channels(tiny):
    """the same recording as 8 kHz stereo: resampled once on the device, then the same path"""
    _, eng, lf, pcm = tiny
    x = pcm[::2].contiguous()
    stereo = torch.stack([x, x], dim=1)
    out = lf.transcribe(stereo, sample_rate=8000, channels=2)
    segs, feat = lf.segment(stereo, sample_rate=8000, channels=2)
    assert len(out) == len(segs) >= 5 and feat.shape[0] == R.num_frames(192000) and out[-1].end_ms <= 12000


def test_cli_vad(tiny, tmp_path):
    """infer.py -w --vad --timestamps in a child process prints the segments, tokens and token times of the in-process transcriber"""
    from m3asr.plan import pack_weights, save_plan
    from m3asr.weights import make_weights
    cfg, eng, lf, pcm = tiny
    plan, wav = str(tmp_path / "m.plan"), str(tmp_path / "a.wav")
    save_plan(plan, cfg, pack_weights(make_weights(cfg, seed=3), cfg))
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.numpy().astype("<i2").tobytes())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "-p", plan, "-w", wav, "--vad", "--vad-max-segment", "150",
                        "--vad-split-search", "60", "--max-batch", "3", "--timestamps"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = lf.transcribe(pcm, timestamps=True)
    lines = r.stdout.splitlines()
    segs = [ln for ln in lines if ln.startswith("seg ") and " ms " in ln]
    assert segs == ["seg %d %d-%d ms greedy: %s" % (i, s.start_ms, s.end_ms, " ".join(str(t) for t in s.tokens)) for i, s in enumerate(want)]
    for i, s in enumerate(want):
        at = lines.index("seg %d greedy times:" % i)
        got = [ln.split() for ln in lines[at + 1:at + 1 + len(s.tokens)]]
        assert [(int(g[0]), int(g[1]), int(g[2])) for g in got] == [(t[0], t[1], t[2]) for t in s.times]
