"""Host tier of the resampler (csrc/resample.hip's host half, m3asr/frontend.py): the sample count and the input span against
the float64 restatement (tests/resample_ref.py), the library's host-built tables against it, the refusals, and the
input-rate window buffer: the 16 kHz windows rebuilt from the spans it hands out are slices of the offline-resampled signal.
No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resample_ref as R
from m3asr import _lib
from m3asr.frontend import AudioWindowBuffer, ResampledWindowBuffer, num_frames, num_resampled, resample_span, resample_tables
from m3asr.serve import next_window_valid

PAIRS = [(8000, 16000), (11025, 16000), (22050, 16000), (32000, 16000), (44100, 16000), (48000, 16000), (47999, 16000),
         (16000, 16000), (16000, 8000)]


def _lengths(ri, ro):
    in_unit = ri // int(np.gcd(ri, ro))
    return sorted({0, 1, max(in_unit - 1, 0), in_unit + 1, 399, 400, 12345, ri, 2 ** 33})


@pytest.mark.parametrize("ri,ro", PAIRS)
def test_count_and_span_equal_the_restatement(ri, ro):
    lib = _lib.load()
    f, e = C.c_int64(0), C.c_int64(0)
    for n in _lengths(ri, ro):
        for flush in (0, 1):
            want = R.num_samples(ri, ro, n, bool(flush))
            assert lib.m3_resample_num_samples(ri, ro, n, flush) == want == num_resampled(n, ri, ro, flush=bool(flush)), (n, flush)
        # the non-flush count never admits an output whose span reaches n
        k = R.num_samples(ri, ro, n, False)
        assert k <= R.num_samples(ri, ro, n, True)
        if k > 0:
            assert R.input_span(ri, ro, k - 1, 1)[1] <= n, n
            assert lib.m3_resample_input_span(ri, ro, k - 1, 1, C.byref(f), C.byref(e)) == 0 and e.value <= n
        for out0, cnt in ((0, 1), (0, max(k, 1)), (max(k - 1, 0), 1), (n, 7), (n + 5, 0), (2 ** 33 + 5, 160)):
            assert lib.m3_resample_input_span(ri, ro, out0, cnt, C.byref(f), C.byref(e)) == 0
            assert (f.value, e.value) == R.input_span(ri, ro, out0, cnt) == resample_span(out0, cnt, ri, ro), (out0, cnt)
    assert R.input_span(ri, ro, 0, 1)[0] < 0 or ri == ro                   # the span may start below 0


@pytest.mark.parametrize("ri", [8000, 44100, 48000])
def test_available_now_is_computable_from_the_count(ri):
    for n in range(1, 2151, 5):                                          # 430 lengths
        k = R.num_samples(ri, 16000, n, False)
        if k:
            assert R.input_span(ri, 16000, 0, k)[1] <= n, n


@functools.lru_cache(maxsize=None)
def _both(ri, ro):
    return resample_tables(ri, ro), R.tables(ri, ro)


@pytest.mark.parametrize("ri,ro", PAIRS)
def test_host_tables_match_the_restatement(ri, ro):
    got, want = _both(ri, ro)
    assert (got["in_unit"], got["out_unit"]) == (want.in_unit, want.out_unit)
    assert np.array_equal(got["first"], want.first) and np.array_equal(got["n"], want.n)
    assert got["weights"].shape == (want.out_unit, want.max_taps) and got["weights"].dtype == np.float32
    worst = 0.0
    for p in range(want.out_unit):
        k = int(want.n[p])
        w32 = want.w[p].astype(np.float32)
        # within 1 fp32 ulp of the rounded float64 value (libm's last bit may move a rounding)
        ulp = np.spacing(np.abs(w32)).astype(np.float64)
        d = np.abs(got["weights"][p, :k].astype(np.float64) - w32.astype(np.float64))
        assert bool((d <= ulp).all()), (p, float(d.max()))
        worst = max(worst, float((d / ulp).max()))
        assert not got["weights"][p, k:].any()                             # padded taps are zeros
        assert abs(float(got["weights"][p].astype(np.float64).sum()) - 1.0) < 1e-3, p
    print("resample tables %d -> %d: %d phases, taps %d..%d, %d floats, worst %.2f ulp" % (
        ri, ro, want.out_unit, int(want.n.min()), want.max_taps, want.floats, worst))
    if ri == ro:
        assert got["first"].tolist() == [0] and got["n"].tolist() == [1] and got["weights"].tolist() == [[1.0]]


def test_table_sizes():
    """phases, taps and floats of the served rates"""
    want = {8000: (2, 12, 13, 25), 11025: (640, 12, 13, 7757), 22050: (320, 16, 17, 5345), 44100: (160, 33, 34, 5345),
            48000: (1, 37, 37, 37), 96000: (1, 73, 73, 73), 47999: (16000, 36, 37, 581807)}
    for ri, (phases, lo, hi, floats) in want.items():
        n = [R._phase(ri, 16000, p)[1] for p in range(phases)]
        assert R.table_shape(ri, 16000) == (phases, hi, floats) and min(n) == lo, ri
        assert _lib.load().m3_resample_tables_bytes(ri, 16000) == 32 + 4 * (-(-2 * phases // 4) * 4 + -(-phases * hi // 4) * 4)


def test_reference_sine_within_kaldi_ripple():
    """1 kHz, amplitude 10000, 48 kHz -> 16 kHz: within 4.0 of the analytic 16 kHz sine away from the edges (the filter's
    pass-band ripple, DC gain 1.00047)."""
    x = 10000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(4800) / 48000.0)
    y, _ = R.resample(x, 48000, 16000)
    t = np.arange(len(y)) / 16000.0
    assert len(y) == 1600 and np.abs(y - 10000.0 * np.sin(2 * np.pi * 1000.0 * t))[20:-20].max() < 4.0


def test_refusals_carry_their_messages():
    lib = _lib.load()
    err = lambda: lib.m3_last_error().decode()
    assert lib.m3_resample_tables_bytes(999, 16000) == 0 and "rate_in=999" in err()
    assert lib.m3_resample_tables_bytes(16000, 384001) == 0 and "rate_out=384001" in err()
    phases, taps, floats = R.table_shape(191999, 16000)
    assert floats > 2 ** 20 and taps <= 512
    assert lib.m3_resample_tables_bytes(191999, 16000) == 0 and "floats" in err() and "16000 phases" in err()
    assert R.table_shape(384000, 1000)[1] > 512
    assert lib.m3_resample_tables_bytes(384000, 1000) == 0 and "max_taps" in err()
    buf = np.zeros(64, np.uint8)
    assert lib.m3_resample_tables_host(999, 16000, buf.ctypes.data) != 0 and "rate_in=999" in err()
    assert lib.m3_resample_tables_host(8000, 16000, None) != 0 and "null" in err()
    assert lib.m3_resample_num_samples(999, 16000, 5, 1) == -1 and "rate_in=999" in err()
    assert lib.m3_resample_tables_bytes(47999, 16000) > 0
    with pytest.raises(_lib.M3Error, match="rate_in=999"):
        resample_tables(999)
    with pytest.raises(_lib.M3Error, match="rate_in=999"):
        AudioWindowBuffer(4, sample_rate=999)
    with pytest.raises(ValueError, match="channels=9"):
        AudioWindowBuffer(4, sample_rate=8000, channels=9)
    # m3_resample checks its arguments before it touches the device: channels = 9 is refused without one
    one = np.zeros(16, np.int64)
    p = one.ctypes.data
    assert lib.m3_resample(p, p, 1, 9, -1, 8, p, p, p, p, 1, 1, p, 1, None) != 0 and "channels=9" in err()
    assert lib.m3_resample(p, p, 1, 2, 2, 8, p, p, p, p, 1, 1, p, 1, None) != 0 and "channel=2" in err()


# ---------------------------------------------------------------- the input-rate window buffer

def _signal(n, channels, seed):
    x = np.round(np.random.default_rng(seed).normal(0, 3000, (n, channels))).astype(np.int16)
    return torch.from_numpy(x)


@pytest.mark.parametrize("rate,channels", [(44100, 2), (44100, 1), (8000, 2), (8000, 1)])
def test_window_buffer_hands_out_slices_of_the_offline_signal(rate, channels):
    """Pieces of [1, 441, 4409, 7, 20000] input samples, a rebase() in the middle: every span, resampled by the float64
    reference at its in0 / out0, is exactly the slice of resample(whole signal) that the window stands for."""
    c, n = 4, {44100: 67638, 8000: 12270}[rate]                            # 24540 samples at 16 kHz: the last window is short
    x = _signal(n, channels, rate + channels)
    mono = R.downmix(x.numpy())
    tab = R.tables(rate, 16000)
    whole, _ = R.resample(mono, rate, 16000, tab=tab)
    assert len(whole) == R.num_samples(rate, 16000, n, True)
    ab = AudioWindowBuffer(c, sample_rate=rate, channels=channels)
    assert isinstance(ab, ResampledWindowBuffer) and ab.window == (4 * c + 2) * 160 + 400
    origin, chunks, windows, pushed = 0, 0, [], 0

    def drain(ended):
        nonlocal origin, chunks
        while True:
            avail = R.num_samples(rate, 16000, pushed, ended) - origin
            v = ab.ready()
            assert v == next_window_valid(num_frames(max(avail, 0)), chunks, c, ended)     # the feature-domain rule
            if v == 0:
                return
            span, in0, n_in, out0, n_out = ab.take()
            assert span.shape == (ab.span, channels) and span.dtype == torch.int16 and not bool(span[n_in:].any())
            assert out0 == origin + 640 * c * chunks and num_frames(n_out) == v and 0 <= n_in <= ab.span
            assert torch.equal(span[:n_in], x[in0:in0 + n_in])
            got, _ = R.resample(R.downmix(span[:n_in].numpy()), rate, 16000, in0=in0, out0=out0, n_out=n_out, tab=tab)
            assert np.array_equal(got, whole[out0:out0 + n_out]), (out0, n_out)
            windows.append((out0, n_out))
            chunks += 1
            if len(windows) == 3:                                          # cut a segment here, as StreamPool._cut does
                ab.rebase()
                origin, chunks = origin + 640 * c * chunks, 0
                assert ab.origin == origin and ab.chunks == 0

    sizes, at, i = [1, 441, 4409, 7, 20000], 0, 0
    while at < n:
        k = min(sizes[i % len(sizes)], n - at)
        ab.push(x[at:at + k] if i % 2 else x[at:at + k].reshape(-1))      # (n, C) and interleaved
        at, pushed, i = at + k, at + k, i + 1
        before = len(windows)
        drain(False)
        assert all(m == ab.window for _, m in windows[before:])           # before the end only FULL windows run
    assert not ab.drained()
    ab.end()
    drain(True)
    assert ab.drained() and len(windows) >= 5 and windows[-1][1] < ab.window     # the short last window ran
    assert windows[3][0] == windows[2][0] + 640 * c                        # the segment after the cut starts at the next window
    assert windows[-1][0] + windows[-1][1] == len(whole)                   # ... and the flushed tail is all there
    assert ab.buf.shape[0] <= ab.span + 20000                              # consumed input is dropped
    with pytest.raises(ValueError):
        ab.push(x[:1])


def test_default_window_buffer_is_unchanged():
    """Constructed with the defaults (given or not) it is the 16 kHz buffer: same fields, same windows on one schedule."""
    x = _signal(11111, 1, 3).reshape(-1)
    got = []
    for ab in (AudioWindowBuffer(4), AudioWindowBuffer(4, torch.int16, 16000, 1)):
        assert type(ab) is AudioWindowBuffer
        assert sorted(vars(ab)) == ["base", "buf", "c", "chunks", "dtype", "ended", "hop", "total", "window"]
        wins = []
        for at in range(0, 11111, 3000):
            ab.push(x[at:at + 3000])
            while ab.ready():
                w, real = ab.take()
                wins.append((w.clone(), real, ab.base, ab.total))
        ab.end()
        while ab.ready():
            w, real = ab.take()
            wins.append((w.clone(), real, ab.base, ab.total))
        got.append(wins)
    assert [r for _, r, _, _ in got[0]] == [3280] * 4
    for (w, r, base, _), k in zip(got[0], range(4)):
        assert torch.equal(w[:r], x[2560 * k:2560 * k + r]) and not bool(w[r:].any()) and base == 2560 * (k + 1)
    assert len(got[0]) == len(got[1]) and all(torch.equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(*got))


class _StubDecoder:
    def __init__(self):
        self.steps = []

    def reset(self, slots=None):
        pass

    def step(self, window, valid):
        self.steps.append((window.clone(), valid.clone()))

    def finish(self, slots=None):
        return [[((b,), 0.0)] for b in slots]


def test_stream_pool_resamples_with_host_stand_ins():
    """The pool's bookkeeping without a device: a resampler and a front end evaluated by the references on the host see, at
    every step, the spans and index entries that reproduce the offline signal; idle slots get n_out = 0."""
    from m3asr.serve import StreamPool
    rate, ch, c, B = 8000, 2, 4, 2
    tab = R.tables(rate, 16000)
    seen = []

    class HostResampler:
        def launch(self, pcm, in0, n_in, out0, n_out, out, stream=None):
            out.zero_()
            for b in range(pcm.shape[0]):
                k, m = int(n_in[b]), int(n_out[b])
                mono = R.downmix(pcm[b, :k * ch].reshape(k, ch).numpy())
                y, _ = R.resample(mono, rate, 16000, in0=int(in0[b]), out0=int(out0[b]), n_out=m, tab=tab)
                out[b, :m] = torch.from_numpy(y).float()
            seen.append((out.clone(), n_out.clone()))
            return out

    def fbank(pcm, n_samples, out=None, out_len=None, stream=None):
        out.zero_()
        return out, out_len

    dec = _StubDecoder()
    pool = StreamPool(dec, B=B, chunk=c, input_dim=40, audio=True, fbank=fbank, sample_rate=rate, channels=ch,
                      resampler=HostResampler())
    x = _signal(4000, ch, 9)
    whole = R.resample(R.downmix(x.numpy()), rate, 16000, tab=tab)[0]
    a = pool.open()
    pool.open()                                                            # an idle neighbour
    pool.push_audio(a, x[:1000])
    assert pool.step() == []
    pool.push_audio(a, x[1000:])
    pool.end(a)
    while pool.pending(a):
        assert pool.step() == [a]
    assert len(seen) == 3 and [int(n[0]) for _, n in seen] == [3280, 3280, 8000 - 2 * 2560]
    for k, (out, n) in enumerate(seen):
        m = int(n[0])
        assert int(n[1]) == 0 and not bool(out[1].any())
        assert np.array_equal(out[0, :m].numpy(), whole[2560 * k:2560 * k + m].astype(np.float32)) and not bool(out[0, m:].any())
    with pytest.raises(ValueError, match="audio=True"):
        StreamPool(_StubDecoder(), B=B, chunk=c, input_dim=40, sample_rate=8000)
