"""The resampler on the device (csrc/resample.hip, m3asr.frontend.Resampler) against the restatement of its contract
(tests/resample_ref.py), and its way into the engine: Engine.infer_audio(sample_rate=), StreamPool(sample_rate=), infer.py -w.

Bounds.  Two references, neither derived from the kernel's output.  (1) The fp32 twin: the kernel's own arithmetic (one fp32
accumulator from 0, taps in ascending j, multiply then add) done with np.float32 scalars on the library's HOST table -- the
kernel must be torch.equal to it.  (2) The float64 restatement with float64 weights: every sample within
(n[p] + 2) * 2^-24 * sum_j |w_j x_j|, the standard bound of an n-term fp32 dot product (n roundings of the running sum and the
products), one more unit for the weight's rounding to fp32 and one for libm's last bit in the table.  Each parity test prints
the worst ratio err / bound before it asserts (run with -s).  Everything that is "the same sample computed elsewhere"
(another batch, another launch window, int16 against float32 input, the streaming path) is torch.equal.
"""
import functools
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G
import resample_ref as R
from m3asr import _lib
from m3asr.frontend import Fbank, Resampler, resample_span, resample_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _speech(n, seed):
    rng = np.random.default_rng(seed)
    x = (np.cumsum(rng.normal(0, 1, n)) * 50 % 20000) - 10000 + rng.normal(0, 200, n)
    return torch.from_numpy(np.round(np.clip(x, -32768, 32767)).astype(np.int16))


def _speech_ch(n, channels, seed):
    return torch.stack([_speech(n, seed + 10 * c) for c in range(channels)], dim=1)          # (n, channels)


@functools.lru_cache(maxsize=None)
def _rs(rate, channels=1, channel=-1, rate_out=16000):
    return Resampler(rate, "cuda:0", rate_out=rate_out, channels=channels, channel=channel)


@functools.lru_cache(maxsize=None)
def _fb(bins=40):
    return Fbank(bins, "cuda:0")


@functools.lru_cache(maxsize=None)
def _tabs(rate, rate_out=16000):
    """(the library's host tables, the float64 restatement's); built once, shared"""
    return resample_tables(rate, rate_out), R.tables(rate, rate_out)


def _twin(mono, rate, in0=0, out0=0, n_out=0):
    t = _tabs(rate)[0]
    return R.resample32(mono, t["first"], t["n"], t["weights"], t["in_unit"], t["out_unit"], in0=in0, out0=out0, n_out=n_out)


def _check_against_references(got, mono, rate, in0=0, out0=0, what=""):
    """got (n_out,) float32 numpy: torch.equal to the fp32 twin, inside the dot-product bound of the float64 reference"""
    n_out = got.shape[0]
    twin = _twin(mono, rate, in0, out0, n_out)
    ref_tab = _tabs(rate)[1]
    y64, mag = R.resample(mono, rate, 16000, in0=in0, out0=out0, n_out=n_out, tab=ref_tab)
    taps = ref_tab.n[(out0 + np.arange(n_out)) % ref_tab.out_unit]
    bound = (taps + 2) * U * mag
    err = np.abs(got.astype(np.float64) - y64)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if n_out else 0.0
    print("resample %s: %d outputs, worst err %.3e, worst err / bound %.3f" % (what, n_out, float(err.max()) if n_out else 0.0, ratio))
    assert np.array_equal(got.view(np.int32), twin.view(np.int32)), what
    assert bool((err <= bound).all()) and float(np.abs(got).max()) > 1000, what


@pytest.mark.parametrize("rate,n", [(8000, 1280), (44100, 4410 + 37), (48000, 2000)])
def test_parity(rate, n):
    x = _speech(n, rate)
    outs = {}
    for dtype in (torch.int16, torch.float32):
        out, n_out = _rs(rate)(x.to(dtype))
        assert tuple(out.shape) == (1, R.num_samples(rate, 16000, n)) and n_out.cpu().tolist() == [out.shape[1]]
        outs[dtype] = out[0].cpu()
        _check_against_references(outs[dtype].numpy(), x.numpy(), rate, what="%d %s" % (rate, dtype))
    assert torch.equal(outs[torch.int16], outs[torch.float32])                   # the same bits from int16 and float32 input


@pytest.mark.parametrize("channels", [2, 3])
def test_channels(channels):
    x = _speech_ch(900, channels, 20 + channels)
    for channel in [-1] + list(range(channels)):
        mono = R.downmix(x.numpy(), channel)
        for dtype in (torch.int16, torch.float32):
            out, n_out = _rs(44100, channels, channel)(x.to(dtype).unsqueeze(0))
            assert n_out.cpu().tolist() == [R.num_samples(44100, 16000, 900)]
            _check_against_references(out[0].cpu().numpy(), mono, 44100, what="%d ch, channel %d, %s" % (channels, channel, dtype))
    # interleaved (B, N * channels) is the same input
    assert torch.equal(_rs(44100, channels)(x.reshape(1, -1))[0], _rs(44100, channels)(x.unsqueeze(0))[0])


def test_same_rate_is_the_identity():
    x = _speech_ch(1003, 2, 31)
    out, n_out = _rs(16000, 2, 0)(x.unsqueeze(0))
    assert n_out.cpu().tolist() == [1003] and torch.equal(out[0].cpu(), x[:, 0].float())
    out, _ = _rs(16000, 2, -1)(x.unsqueeze(0))
    assert torch.equal(out[0].cpu(), torch.from_numpy(R.downmix(x.numpy())))


def _launch(rs, pcm, in0, n_in, out0, n_out, N_out):
    """one launch on fresh dense operands -> out (B, N_out) on the CPU"""
    B = pcm.shape[0]
    per16 = 16 // pcm.element_size()
    dev = torch.zeros(B, max(-(-pcm.shape[1] // per16) * per16, per16), dtype=pcm.dtype, device="cuda")
    dev[:, :pcm.shape[1]] = pcm.cuda()
    v = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    out = torch.full((B, N_out), float("nan"), device="cuda")
    rs.launch(dev, v(in0, torch.int64), v(n_in, torch.int32), v(out0, torch.int64), v(n_out, torch.int32), out)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_ragged_guarded_strided(dtype):
    """B = 3, lengths [4410, 0, 1], pcm and out row-strided inside guard buffers: nothing outside [0, N_out) of a row is written,
    [n_out, N_out) is zeros, no guard sample is read (it would change a value), each row equals the row run alone."""
    lib, rs = _lib.load(), _rs(44100)
    lengths, N_out = [4410, 0, 1], 1603
    x = _speech(4416, 44).to(dtype)
    rows = torch.stack([x, x.flip(0), x.roll(7)])
    pcm = G.strided_in(rows, int_guard=32767)
    want_n = [R.num_samples(44100, 16000, k) for k in lengths]
    assert want_n == [1600, 0, 1]
    v = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    zero, n_in, n_out = v([0, 0, 0], torch.int64), v(lengths, torch.int32), v(want_n, torch.int32)
    out = G.strided_out(3, N_out, ld=1640)
    _lib.check(lib.m3_resample(rs.tables.data_ptr(), pcm.view.data_ptr(), int(dtype == torch.int16), 1, -1, pcm.ld, zero.data_ptr(),
                               n_in.data_ptr(), zero.data_ptr(), n_out.data_ptr(), 3, N_out, out.view.data_ptr(), out.ld, None),
               "m3_resample")
    torch.cuda.synchronize()
    out.check("out")
    assert not bool(out.untouched().any())
    got = G.dense(out.view).cpu()
    for b, (k, m) in enumerate(zip(lengths, want_n)):
        assert not bool(got[b, m:].any()) and bool(torch.isfinite(got[b]).all())
        alone, n_alone = rs(rows[b, :k])
        assert n_alone.cpu().tolist() == [m] and torch.equal(alone[0].cpu(), got[b, :m])
    _check_against_references(got[0, :1600].numpy(), rows[0, :4410].numpy(), 44100, what="ragged row 0 %s" % dtype)
    # n_in beyond the row and n_out beyond N_out are clamped; an out0 below 0 gives an empty row
    out2 = _launch(rs, rows[:1], [0], [99999], [0], [99999], 1600)
    assert torch.equal(out2[0, :1590], got[0, :1590]) and not torch.equal(out2[0], got[0, :1600])   # (the last taps now see samples 4410..4415)
    assert not bool(_launch(rs, rows[:1], [0], [4410], [-1], [100], 128).any())


def test_chunk_invariance():
    """44100 -> 16000: outputs [0, 1600) from one launch, and from launches that cut them at [1, 159, 160, 161, 1119], each
    given only its own input span, at nonzero in0 / out0."""
    rs, n = _rs(44100), 4410
    x = _speech(n, 45)
    whole = _launch(rs, x.unsqueeze(0), [0], [n], [0], [1600], 1600)[0]
    _check_against_references(whole.numpy(), x.numpy(), 44100, what="whole")
    cuts, parts = [0, 1, 159, 160, 161, 1119, 1600], []
    for o0, o1 in zip(cuts[:-1], cuts[1:]):
        lo, hi = resample_span(o0, o1 - o0, 44100)
        lo, hi = max(lo, 0), min(hi, n)
        assert o0 < 159 or lo > 0
        parts.append(_launch(rs, x[lo:hi].clone().unsqueeze(0), [lo], [hi - lo], [o0], [o1 - o0], o1 - o0)[0])
    assert torch.equal(torch.cat(parts), whole)
    # several cuts as the rows of ONE launch (different in0 / out0 per row) are the same samples again
    spans = [(max(resample_span(o0, o1 - o0, 44100)[0], 0), min(resample_span(o0, o1 - o0, 44100)[1], n)) for o0, o1 in zip(cuts[3:-1], cuts[4:])]
    width = max(hi - lo for lo, hi in spans)
    rows = torch.zeros(3, width, dtype=torch.int16)
    for b, (lo, hi) in enumerate(spans):
        rows[b, :hi - lo] = x[lo:hi]
    counts = [o1 - o0 for o0, o1 in zip(cuts[3:-1], cuts[4:])]
    batch = _launch(rs, rows, [lo for lo, _ in spans], [hi - lo for lo, hi in spans], cuts[3:-1], counts, 1000)
    for b, (o0, m) in enumerate(zip(cuts[3:-1], counts)):
        assert torch.equal(batch[b, :m], whole[o0:o0 + m]) and not bool(batch[b, m:].any())


@pytest.mark.parametrize("rate", [44100, 48000])
def test_far_into_a_session(rate):
    """out0 = 2^33 + 5: twelve hours of 48 kHz pass 2^31 input samples; every absolute index is 64-bit."""
    out0, m = 2 ** 33 + 5, 200
    lo, hi = resample_span(out0, m, rate)
    assert lo > 2 ** 33 and 300 < hi - lo < 1000
    x = _speech(hi - lo, 46)
    got = _launch(_rs(rate), x.unsqueeze(0), [lo], [hi - lo], [out0], [m], m)[0]
    _check_against_references(got.numpy(), x.numpy(), rate, in0=lo, out0=out0, what="%d at 2^33 + 5" % rate)


def test_device_tables_are_the_host_tables():
    for rate in (8000, 44100, 47999):
        assert torch.equal(_rs(rate).tables.cpu(), torch.from_numpy(resample_tables(rate)["image"]))


def test_bad_arguments_are_refused():
    lib, rs = _lib.load(), _rs(8000)
    pcm = torch.zeros(1, 800, dtype=torch.int16, device="cuda")
    out = torch.zeros(1, 160, device="cuda")
    i64, i32 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(tables=rs.tables.data_ptr(), p=pcm, ch=1, k=-1, ld_pcm=800, N_out=160, ld_out=160, o=out):
        return lib.m3_resample(tables, p.data_ptr(), 1, ch, k, ld_pcm, i64.data_ptr(), i32.data_ptr(), i64.data_ptr(), i32.data_ptr(),
                               1, N_out, o.data_ptr(), ld_out, None)

    assert call() == 0
    assert call(ch=9) != 0 and "channels=9" in _lib.last_error()
    assert call(ch=2, k=2) != 0 and "channel=2" in _lib.last_error()
    assert call(ld_pcm=804) != 0 and "ld_pcm" in _lib.last_error()
    assert call(ld_out=159) != 0 and "ld_out" in _lib.last_error()
    assert call(N_out=-1, ld_out=160) != 0 and "N_out" in _lib.last_error()
    assert call(p=pcm[:, 1:]) != 0 and "aligned" in _lib.last_error()
    assert call(o=out[:, 1:], N_out=100) != 0 and "aligned" in _lib.last_error()
    assert call(tables=None) != 0 and "null" in _lib.last_error()
    tables = torch.empty(4096, dtype=torch.uint8, device="cuda")
    assert lib.m3_resample_tables_init(999, 16000, tables.data_ptr(), None) != 0 and "rate_in=999" in _lib.last_error()
    assert lib.m3_resample_tables_init(8000, 16000, None, None) != 0 and "tables" in _lib.last_error()
    with pytest.raises(_lib.M3Error, match="rate_in=999"):
        Resampler(999, "cuda:0")
    with pytest.raises(ValueError, match="channels=9"):
        Resampler(8000, "cuda:0", channels=9)
    with pytest.raises(ValueError, match="3 channels"):
        rs(torch.zeros(1, 10, 3))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- into the engine

def test_infer_audio_at_8k_equals_infer_on_the_resampled_features(golden):
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg, _ = golden("tiny")
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=3))
    pcm16 = torch.stack([_speech(8000, 7), _speech(8000, 8)])
    eng.infer_audio(pcm16, torch.tensor([8000, 5555]))
    assert not getattr(eng, "_resamplers", None)                                   # the defaults create no resampler
    pcm8 = torch.stack([_speech(4000, 7), _speech(4000, 8)])
    n = torch.tensor([4000, 2777])
    res, n_out = _rs(8000)(pcm8, n)
    assert n_out.cpu().tolist() == [8000, 5554]
    feat, flen = _fb(cfg.input_dim)(res, n_out)
    assert tuple(feat.shape) == (2, 48, cfg.input_dim) and flen.cpu().tolist() == [48, 33]
    want = eng.infer(feat, flen).cpu().clone()
    got = eng.infer_audio(pcm8, n, sample_rate=8000).cpu().clone()
    assert torch.equal(got, want) and float(want.abs().max()) > 0
    assert list(eng._resamplers) == [(8000, 1, -1)]
    assert torch.equal(eng.infer_audio(pcm8.float().cuda(), n, sample_rate=8000).cpu(), want)
    assert list(eng._resamplers) == [(8000, 1, -1)]                                # cached per (rate, channels, channel)
    stereo = torch.stack([pcm8, pcm8], dim=2)                                      # both channels alike: the mean is the channel
    assert torch.equal(eng.infer_audio(stereo, n, sample_rate=8000, channels=2).cpu(), want)
    assert torch.equal(eng.infer_audio(stereo, n, sample_rate=8000, channels=2, channel=1).cpu(), want)


@pytest.fixture(scope="module")
def causal_engine(golden):
    import dataclasses
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg, _ = golden("causal")
    cfg = dataclasses.replace(cfg, static_chunk_size=4, num_decoding_left_chunks=2)
    return Engine.from_state_dict(cfg, make_weights(cfg, seed=41), packed_rows=False)


class _Tap:
    """A decoder that records the frames standing in the encoder's window buffer at every step."""

    def __init__(self, dec):
        self.dec, self.st, self.seen = dec, dec.st, []

    def step(self, window, valid):
        self.dec.step(window, valid)
        self.st.eng.stream.synchronize()
        self.seen.append((self.st.feat.cpu().clone(), valid.clone()))

    def __getattr__(self, name):
        return getattr(self.dec, name)


def _drive(pool, push, plan, pieces):
    """plan: [(first step, samples or frames)]; pieces: sizes pushed per step, cycled.  -> n-best per session."""
    sids, sent, results, step = {}, {}, {}, 0
    while len(results) < len(plan):
        assert step < 200, "schedule does not end"
        for i, (s0, x) in enumerate(plan):
            if step >= s0 and i not in sids:
                sids[i], sent[i] = pool.open(), 0
            if i in sids and i not in results and sent[i] < x.shape[0]:
                k = min(pieces[(step + i) % len(pieces)], x.shape[0] - sent[i])
                push(sids[i], x[sent[i]:sent[i] + k])
                sent[i] += k
                if sent[i] == x.shape[0]:
                    pool.end(sids[i])
        pool.step()
        for i in list(sids):
            if i not in results and sent[i] == plan[i][1].shape[0] and not pool.pending(sids[i]):
                results[i] = pool.close(sids[i])
        step += 1
    return [results[i] for i in range(len(plan))]


def test_streaming_identity(causal_engine):
    """1 s of 44.1 kHz stereo through StreamPool(audio=True, sample_rate=44100, channels=2) in uneven pieces: at every chunk
    the frames in the encoder's window buffer are the frames of Fbank(Resampler(whole signal)), which a feature-mode pool is
    given, and the n-best is the same; a second session that starts three steps late gives what it gives alone."""
    from m3asr.decode import StreamingCtcDecoder
    from m3asr.serve import StreamPool
    eng, B, Tp = causal_engine, 2, 64
    fb, rs = _fb(eng.cfg.input_dim), _rs(44100, 2)
    xa, xb = _speech_ch(44100, 2, 5), _speech_ch(25000, 2, 6)
    fa, fb_ = (fb(*rs(x.unsqueeze(0)))[0][0].cpu() for x in (xa, xb))
    assert fa.shape[0] == 98

    def pools():
        ta = _Tap(StreamingCtcDecoder(eng.streaming(B, Tp, independent=True), beam=4))
        tf = _Tap(StreamingCtcDecoder(eng.streaming(B, Tp, independent=True), beam=4))
        return ta, StreamPool(ta, audio=True, sample_rate=44100, channels=2), tf, StreamPool(tf)

    ta, audio, tf, feats = pools()
    got = _drive(audio, audio.push_audio, [(0, xa)], [1, 441, 4409, 20000])
    want = _drive(feats, feats.push, [(0, fa)], [50])
    assert len(ta.seen) == len(tf.seen) == 6 and got == want and len(want[0]) > 1
    for (f, v), (g, w) in zip(ta.seen, tf.seen):
        assert torch.equal(v, w) and torch.equal(f, g)
    assert ta.seen[-1][1].tolist()[0] < 19                                            # the short last window ran too
    alone_b = _drive(feats, feats.push, [(0, fa[:0]), (0, fb_)], [50])[1]              # alone, in slot 1 (an empty session holds slot 0)
    ta, audio, _, _ = pools()
    both = _drive(audio, audio.push_audio, [(0, xa), (3, xb)], [6000, 333, 3528])
    assert both[0] == want[0] and both[1] == alone_b and both[0] != both[1]


def test_cli_wav_at_44k_stereo(golden, tmp_path):
    """infer.py -w on a 44.1 kHz stereo wav prints the same output shape and sum as -i on the features made in-process from the
    same samples (a fresh child each)."""
    from m3asr.plan import pack_weights, save_plan
    from m3asr.weights import make_weights
    cfg, _ = golden("tiny")
    plan, wav, npy = (str(tmp_path / k) for k in ("m.plan", "a.wav", "feat.npy"))
    save_plan(plan, cfg, pack_weights(make_weights(cfg, seed=3), cfg))
    x = _speech_ch(22050, 2, 9)
    with wave.open(wav, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(x.numpy().astype("<i2").tobytes())
    np.save(npy, _fb(cfg.input_dim)(*_rs(44100, 2)(x.unsqueeze(0)))[0].cpu().numpy())

    def run(*src):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "-p", plan, *src], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.startswith("outputs.shape:") or ln.startswith("outputs.sum:")]

    a, b = run("-w", wav), run("-i", npy)
    assert len(a) == 2 and a == b and a[0].startswith("outputs.shape:(1, 11,"), (a, b)
