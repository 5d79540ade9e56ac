"""Host tier of the audio front end (m3asr/frontend.py, StreamPool(audio=True)): frame arithmetic, the reference itself on
inputs with a known answer, the library's host-built tables against the reference's independently computed window and mel
weights, the sample-domain window buffer against the frame-domain one, and the pool's audio mode with a stub decoder.  No GPU."""
import numpy as np
import pytest
import torch

import fbank_ref
from m3asr._lib import M3Error
from m3asr.frontend import AudioWindowBuffer, fbank_tables, num_frames
from m3asr.serve import StreamPool, WindowBuffer


def test_num_frames():
    want = {0: 0, 399: 0, 400: 1, 559: 1, 560: 2, 16000: 98}
    for n, f in want.items():
        assert num_frames(n) == f and fbank_ref.num_frames(n) == f, n
    from m3asr import _lib
    assert [_lib.load().m3_fbank_num_frames(n) for n in want] == list(want.values())


def test_reference_silence_and_dc_hit_the_floor():
    floor = np.log(np.float64(fbank_ref.FLT_EPSILON))
    for x in (np.zeros(2000, np.int16), np.full(2000, 1234, np.int16), np.full(2000, -20000.0, np.float32)):
        for dtype in (np.float64, np.float32):
            got = fbank_ref.fbank_ref(x, 40, dtype)
            assert got.shape == (11, 40) and bool((got == dtype(floor)).all()), (x.dtype, dtype)


def test_reference_sine_peaks_in_bin_13():
    """1 kHz, amplitude 10000, 1 s: mel bin 13 of 40 (centre 986 Hz) carries the tone."""
    t = np.arange(16000) / 16000.0
    got = fbank_ref.fbank_ref(10000.0 * np.sin(2 * np.pi * 1000.0 * t), 40)
    assert got.shape == (98, 40) and int(got.mean(axis=0).argmax()) == 13


@pytest.mark.parametrize("bins", [23, 40, 80, 128])
def test_tables_match_the_reference(bins):
    """The library's tables (float64 on the host, rounded once) against the reference's formulas: float32 rounding apart."""
    tab = fbank_tables(bins)
    half_ulp = 2.0 ** -24                                   # all entries are <= 1 in magnitude
    assert np.abs(tab["window"].astype(np.float64) - fbank_ref.povey_window()).max() <= half_ulp
    want = fbank_ref.mel_weights(bins)
    assert tab["mel"].shape == want.shape and np.abs(tab["mel"].astype(np.float64) - want).max() <= half_ulp
    assert np.array_equal(tab["mel"] > 0, want.astype(np.float32) > 0)            # the same FFT bins in the same triangles
    assert int((want > 0).sum(axis=0).max()) <= 2                                 # a bin touches at most two triangles
    q = np.arange(256)
    assert np.abs(tab["twiddle256"] - np.exp(-2j * np.pi * q / 256)).max() <= 2 * half_ulp
    assert np.abs(tab["twiddle512"] - np.exp(-2j * np.pi * q / 512)).max() <= 2 * half_ulp
    assert np.float32(tab["log_floor"]) == fbank_ref.LOG_FLOOR


def test_tables_reject_bad_options():
    from m3asr import _lib
    lib = _lib.load()
    assert lib.m3_fbank_tables_bytes(129) == 0 and b"num_mel_bins" in lib.m3_last_error()
    assert lib.m3_fbank_tables_bytes(0) == 0
    buf = np.zeros(lib.m3_fbank_tables_bytes(40), np.uint8)
    assert lib.m3_fbank_tables_host(40, 8000.0, 20.0, 4000.0, buf.ctypes.data) != 0 and b"sample_rate" in lib.m3_last_error()
    assert lib.m3_fbank_tables_host(40, 16000.0, 20.0, 9000.0, buf.ctypes.data) != 0 and b"high_freq" in lib.m3_last_error()
    with pytest.raises(M3Error):
        fbank_tables(129)


def _signal(n, seed):
    return torch.from_numpy(np.round(np.random.default_rng(seed).normal(0, 3000, n)).astype(np.int16))


def _pieces(total, sizes):
    sent, i = 0, 0
    while sent < total:
        n = min(sizes[i % len(sizes)], total - sent)
        yield sent, n
        sent, i = sent + n, i + 1


@pytest.mark.parametrize("n", [399, 400, 3000, 11111])
def test_audio_window_buffer_cuts_what_window_buffer_cuts(n):
    """chunk 4: the windows AudioWindowBuffer hands out, featurised by the reference, are the windows WindowBuffer hands out
    when it is fed fbank_ref(whole signal): same count, same `valid`, the short last window included."""
    c, bins = 4, 40
    x = _signal(n, n)
    whole = torch.from_numpy(fbank_ref.fbank_ref(x.numpy(), bins))
    wb = WindowBuffer(c, bins)
    wb.push(whole.float())
    wb.end()
    want = []
    while wb.ready():
        w, v = wb.take()
        want.append((w.clone(), v))
    ab, got = AudioWindowBuffer(c), []
    assert ab.window == (4 * c + 2) * 160 + 400

    def drain():
        while ab.ready():
            v = ab.ready()
            s, real = ab.take()
            assert num_frames(real) == v and s.shape == (ab.window,) and s.dtype == torch.int16
            assert not bool(s[real:].any())
            f = torch.zeros(4 * c + 3, bins)
            f[:v] = torch.from_numpy(fbank_ref.fbank_ref(s[:real].numpy(), bins)).float()
            got.append((f, v))

    for at, k in _pieces(n, [1, 159, 160, 401, 5000]):
        ab.push(x[at:at + k])
        before = len(got)
        drain()
        assert all(v == 4 * c + 3 for _, v in got[before:])                   # before the end only FULL windows run
    assert not ab.drained()
    ab.end()
    drain()
    assert ab.drained()
    assert [v for _, v in got] == [v for _, v in want]
    for (f, _), (w, _) in zip(got, want):
        assert torch.equal(f, w)
    assert ab.buf.shape[0] <= ab.window + 5000                                 # consumed samples are dropped
    with pytest.raises(ValueError):
        ab.push(x[:1])
    assert len(want) == {399: 0, 400: 0, 3000: 1, 11111: 4}[n]
    if n == 3000:
        assert want[-1][1] == 17                                               # the short last window


def test_audio_window_buffer_rounds_float_samples():
    ab = AudioWindowBuffer(4)
    ab.push(torch.tensor([0.4, -0.6, 40000.0, -40000.0]))
    assert ab.buf.tolist() == [0, -1, 32767, -32768]


class _StubDecoder:
    def __init__(self):
        self.steps, self.resets, self.frames = [], [], {}

    def reset(self, slots=None):
        self.resets.append(list(slots))
        for b in slots:
            self.frames[b] = 0

    def step(self, window, valid):
        self.steps.append((window.clone(), valid.clone()))
        for b, v in enumerate(valid.tolist()):
            self.frames[b] = self.frames.get(b, 0) + v

    def partial(self, slots=None):
        return [((b,), float(self.frames[b])) for b in slots], [[self.frames[b]] for b in slots]

    def finish(self, slots=None):
        return [[((b,), float(self.frames[b]))] for b in slots]


def _host_fbank(bins):
    """What StreamPool needs of a front end, evaluated by the reference on the host."""
    calls = []

    def fbank(pcm, n_samples, out=None, out_len=None, stream=None):
        calls.append(n_samples.tolist())
        out.zero_()
        for b, n in enumerate(n_samples.tolist()):
            f = fbank_ref.fbank_ref(pcm[b, :n].numpy(), bins)
            out[b, :f.shape[0]] = torch.from_numpy(f).float()
            out_len[b] = f.shape[0]
        return out, out_len

    fbank.calls = calls
    return fbank


def test_stream_pool_audio_mode():
    c, bins, B = 4, 40, 2
    window, wsamples = 4 * c + 3, (4 * c + 2) * 160 + 400
    dec, fb = _StubDecoder(), _host_fbank(bins)
    pool = StreamPool(dec, B=B, chunk=c, input_dim=bins, audio=True, fbank=fb)
    a, b_ = pool.open(), pool.open()
    assert dec.resets == [[0], [1]]
    with pytest.raises(M3Error):
        pool.open()
    with pytest.raises(ValueError, match="push_audio"):
        pool.push(a, torch.zeros(3, bins))
    assert pool.step() == [] and dec.steps == []
    xa, xb = _signal(wsamples + 640 * c, 1), _signal(400 + 160 * 8, 2)              # a: two full windows; b: 9 frames, ended
    pool.push_audio(a, xa[:wsamples - 1])
    pool.push_audio(b_, xb)
    pool.end(b_)
    assert not pool.pending(a) and pool.pending(b_)
    assert pool.step() == [b_]
    win, valid = dec.steps[-1]
    assert valid.tolist() == [0, 9] and fb.calls[-1] == [0, xb.shape[0]]
    want_b = torch.from_numpy(fbank_ref.fbank_ref(xb.numpy(), bins)).float()
    assert torch.equal(win[1, :9], want_b) and not bool(win[1, 9:].any()) and not bool(win[0].any())
    pool.push_audio(a, xa[wsamples - 1:])
    assert pool.step() == [a] and pool.step() == [a] and pool.step() == []
    want_a = torch.from_numpy(fbank_ref.fbank_ref(xa.numpy(), bins)).float()
    assert dec.steps[-2][1].tolist() == [window, 0] and dec.steps[-1][1].tolist() == [window, 0]
    assert torch.equal(dec.steps[-2][0][0], want_a[:window]) and torch.equal(dec.steps[-1][0][0], want_a[4 * c:4 * c + window])
    assert not bool(dec.steps[-1][0][1].any())                                       # the idle slot's rows are zeroed
    assert pool.close(b_) == [((1,), 9.0)] and pool.free_slots() == 1
    with pytest.raises(KeyError):
        pool.push_audio(b_, xb)
    d = pool.open()                                                                  # the freed slot again, restarted
    assert pool.slot_of(d) == 1 and dec.resets[-1] == [1] and dec.frames[1] == 0
    pool.push_audio(d, xb.float())                                                   # float32 in the int16 range
    pool.end(d)
    assert pool.step() == [d] and torch.equal(dec.steps[-1][0][1, :9], want_b)
    for s in (a, d):
        pool.close(s)
    assert pool.free_slots() == B
    feature_pool = StreamPool(_StubDecoder(), B=B, chunk=c, input_dim=bins)
    s = feature_pool.open()
    with pytest.raises(ValueError, match="audio=True"):
        feature_pool.push_audio(s, xb)
