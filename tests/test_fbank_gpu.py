"""The log-Mel front end on the device (csrc/fbank.hip, m3asr/frontend.py) against the float64 restatement of its contract
(tests/fbank_ref.py), and its way into the engine: Engine.infer_audio, StreamPool(audio=True), infer.py -w.

Bounds.  The yardstick for "a correct float32 implementation" is the SAME evaluation done in float32 on the CPU (numpy /
scipy, another FFT and another summation order): e32 = max |cpu32 - cpu64| on the test's own input.  The kernel must be
within max(8 e32, 1e-5) of the float64 reference in the log domain: a 512-point FFT and a <= 40-term sum in another rounding
order differ from numpy's by a small constant factor, while a wrong twiddle, window exponent, pre-emphasis order or bin mapping
shows at >= 1e-2.  No bound is derived from the kernel's output; every parity test prints the kernel's error, e32 and the
bound before it asserts (run with -s to see them).  On the CPU e32 is 1.7e-5 (noise), about 1.5e-4 (tones) and 5.6e-6
(speech-like), and a float32 emulation of the kernel's exact arithmetic (same tables, same butterfly order) is within 1.1e-5
of the float64 reference on the noise case.
Everything that is "the same frame computed elsewhere" (another batch, another position, the streaming path) is torch.equal.
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

import fbank_ref
import guarded as G
from m3asr import _lib
from m3asr.frontend import Fbank, num_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = (400, 1999, 4000)


@functools.lru_cache(maxsize=None)
def _fb(bins=40):
    return Fbank(bins, "cuda:0")


@functools.lru_cache(maxsize=None)
def _case(name):
    """One seeded signal of 4000 samples per case (float64, in the int16 value range)."""
    rng = np.random.default_rng({"noise": 11, "tones": 12, "speech": 13, "sine": 14}[name])
    t = np.arange(4000) / 16000.0
    if name == "noise":
        return rng.normal(0, 3000, 4000)
    if name == "tones":
        return 8000 * np.sin(2 * np.pi * 440 * t) + 4000 * np.sin(2 * np.pi * 3100 * t) + rng.normal(0, 30, 4000)
    if name == "speech":
        return np.round(np.clip((np.cumsum(rng.normal(0, 1, 4000)) * 50 % 20000) - 10000 + rng.normal(0, 200, 4000), -32768, 32767))
    t = np.arange(16000) / 16000.0
    return 10000.0 * np.sin(2 * np.pi * 1000.0 * t)


def _as(x, dtype):
    """the signal as the kernel's input of that dtype (int16: rounded), numpy"""
    return np.round(x).astype(np.int16) if dtype == "int16" else x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _refs(name, dtype, bins, n):
    """(cpu64, cpu32) log-Mel of the first n samples of a case; computed once, shared, never written to."""
    x = _as(_case(name), dtype)[:n]
    r64, r32 = fbank_ref.fbank_ref(x, bins), fbank_ref.fbank_ref(x, bins, np.float32)
    r64.setflags(write=False)
    r32.setflags(write=False)
    return r64, r32


def _batch(rows, dtype):
    """rows of different lengths side by side (zeros behind each) -> (pcm (B, N) tensor, n_samples list)"""
    N = max(len(r) for r in rows)
    pcm = np.zeros((len(rows), N), dtype=np.int16 if dtype == "int16" else np.float32)
    for b, r in enumerate(rows):
        pcm[b, :len(r)] = r
    return torch.from_numpy(pcm), [len(r) for r in rows]


def _check_parity(name, dtype, bins, T=24):
    x = _as(_case(name), dtype)
    pcm, n = _batch([x[:k] for k in RAGGED], dtype)
    out = torch.full((len(RAGGED), T, bins), float("nan"), device="cuda")
    feat, flen = _fb(bins)(pcm, n, out=out)
    torch.cuda.synchronize()
    got = feat.cpu().numpy().astype(np.float64)
    assert flen.cpu().tolist() == [min(num_frames(k), T) for k in RAGGED]
    err = e32 = 0.0
    for b, k in enumerate(RAGGED):
        r64, r32 = _refs(name, dtype, bins, k)
        f = min(r64.shape[0], T)
        assert f == min(num_frames(k), T)
        err = max(err, float(np.abs(got[b, :f] - r64[:f]).max()))
        e32 = max(e32, float(np.abs(r32[:f].astype(np.float64) - r64[:f]).max()))
        assert not got[b, f:].any(), "frames past feat_len must be exactly zero"       # (the buffer held NaN)
    bound = max(8 * e32, 1e-5)
    print("fbank parity %s %s bins=%d: kernel err %.3e, e32 %.3e, bound %.3e" % (name, dtype, bins, err, e32, bound))
    assert np.isfinite(got).all() and err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("name", ["noise", "tones", "speech"])
def test_parity_log_domain(name, dtype):
    _check_parity(name, dtype, 40)


@pytest.mark.parametrize("bins", [23, 80, 128])
def test_other_bin_counts(bins):
    _check_parity("noise", "int16", bins)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_parity_pure_tone(dtype):
    """1 kHz, amplitude 10000, 1 s.  Bins far from the tone are ill-conditioned in float32 (cpu32 and cpu64 differ by 0.019
    in the log domain there), so ENERGIES are compared, per frame with the maximum over the frame's bins; the three outputs
    (kernel, cpu32, cpu64) are turned into energies the same way, exp in float64."""
    x = _as(_case("sine"), dtype)
    feat, flen = _fb()(torch.from_numpy(x))
    got = np.exp(feat[0].cpu().numpy().astype(np.float64))
    r64, r32 = _refs("sine", dtype, 40, 16000)
    assert flen.cpu().tolist() == [98] and got.shape == r64.shape == (98, 40)
    e_ref, e_32 = np.exp(r64), np.exp(r32.astype(np.float64))
    err, bound = np.abs(got - e_ref).max(axis=1), 8 * np.abs(e_32 - e_ref).max(axis=1)
    worst = int((err / bound).argmax())
    print("fbank tone %s: worst frame %d energy err %.3e, bound %.3e" % (dtype, worst, err[worst], bound[worst]))
    assert bool((err <= bound).all()), (worst, err[worst], bound[worst])
    assert int(feat[0].mean(dim=0).argmax()) == 13


def test_edges_short_rows_silence_and_tail():
    x = _as(_case("noise"), "int16")
    pcm, n = _batch([x[:0], x[:399], np.zeros(2000, np.int16), x[:2000]], "int16")
    out = torch.full((4, 13, 40), float("nan"), device="cuda")
    feat, flen = _fb()(pcm, n, out=out)
    assert feat.data_ptr() == out.data_ptr() and flen.cpu().tolist() == [0, 0, 11, 11]
    feat = feat.cpu()
    assert not bool(feat[0].any()) and not bool(feat[1].any())                      # no frame: an all-zero row block
    assert bool((feat[2, :11] == float(fbank_ref.LOG_FLOOR)).all())                 # silence: exactly log(FLT_EPSILON)
    assert not bool(feat[2:, 11:].any()) and bool(torch.isfinite(feat).all())       # the tail of a NaN-filled buffer: zeros
    r64, r32 = _refs("noise", "int16", 40, 2000)
    assert float(np.abs(feat[3, :11].double().numpy() - r64).max()) <= max(8 * float(np.abs(r32 - r64).max()), 1e-5)
    # n_samples beyond the row is clamped to the row; T smaller than the frames there are: feat_len is clamped to T
    feat2, flen2 = _fb()(pcm[3:, :2000], [5000], out=torch.empty(1, 5, 40, device="cuda"))
    assert flen2.cpu().tolist() == [5] and torch.equal(feat2[0].cpu(), feat[3, :5])
    # fewer than 400 samples everywhere: no frame at all
    feat3, flen3 = _fb()(pcm[:, :399])
    assert tuple(feat3.shape) == (4, 0, 40) and flen3.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_strided_guarded_operands(dtype):
    """ld_feat > bins and a row-strided pcm, both inside guard buffers: nothing outside the rows' payload is written, no guard
    sample is read (a consumed NaN / guard sample would change the result)."""
    lib, fb = _lib.load(), _fb()
    x = torch.from_numpy(_as(_case("noise"), "int16")).to(dtype)
    B, T, N = 3, 12, 2000                                                           # 11 real frames + 1 zero frame per row
    rows = torch.stack([x[:N], x[1000:1000 + N], x[2000:2000 + N]])
    pcm = G.strided_in(rows, int_guard=32767)
    n_dev = torch.tensor([N, 1999, 400], dtype=torch.int32, device="cuda")
    out = G.strided_out(B * T, 40, ld=56)
    flen = G.flat_out((B,), torch.int32)
    _lib.check(lib.m3_fbank(fb.tables.data_ptr(), pcm.view.data_ptr(), int(dtype == torch.int16), pcm.ld, n_dev.data_ptr(), B, T,
                            40, out.view.data_ptr(), out.ld, flen.view.data_ptr(), None), "m3_fbank")
    torch.cuda.synchronize()
    out.check("feat")
    flen.check("feat_len")
    assert not bool(out.untouched().any()) and flen.view.cpu().tolist() == [11, 10, 1]
    want, _ = fb(rows, n_dev, out=torch.empty(B, T, 40, device="cuda"))
    assert torch.equal(G.dense(out.view).view(B, T, 40), want) and bool(torch.isfinite(want).all())


def test_bad_arguments_are_refused():
    lib, fb = _lib.load(), _fb()
    pcm = torch.zeros(1, 800, dtype=torch.int16, device="cuda")
    n = torch.tensor([800], dtype=torch.int32, device="cuda")
    out, flen = torch.zeros(1, 3, 160, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(bins=40, ld_pcm=800, ld_feat=160, p=pcm, is16=1):
        return lib.m3_fbank(fb.tables.data_ptr(), p.data_ptr(), is16, ld_pcm, n.data_ptr(), 1, 3, bins, out.data_ptr(), ld_feat,
                            flen.data_ptr(), None)

    assert call() == 0
    assert call(bins=129) != 0 and "num_mel_bins" in _lib.last_error()
    assert call(ld_feat=39) != 0 and "ld_feat" in _lib.last_error()
    assert call(ld_pcm=804) != 0 and "ld_pcm" in _lib.last_error()
    assert call(p=pcm[:, 1:]) != 0 and "aligned" in _lib.last_error()
    assert lib.m3_fbank(None, pcm.data_ptr(), 1, 800, n.data_ptr(), 1, 3, 40, out.data_ptr(), 160, flen.data_ptr(), None) != 0
    assert "null" in _lib.last_error()
    tables = torch.empty(lib.m3_fbank_tables_bytes(40), dtype=torch.uint8, device="cuda")
    assert lib.m3_fbank_tables_init(40, 8000.0, 20.0, 4000.0, tables.data_ptr(), None) != 0 and "sample_rate" in _lib.last_error()
    assert lib.m3_fbank_tables_init(129, 16000.0, 20.0, 8000.0, tables.data_ptr(), None) != 0 and "num_mel_bins" in _lib.last_error()
    with pytest.raises(_lib.M3Error, match="num_mel_bins"):
        Fbank(129, "cuda:0")
    torch.cuda.synchronize()


def test_device_tables_are_the_host_tables():
    from m3asr.frontend import fbank_tables
    assert torch.equal(_fb(80).tables.cpu(), torch.from_numpy(fbank_tables(80)["image"]))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_position_independence(dtype):
    """A frame's bits depend on its 400 samples only: the same signal alone, as row 2 of a larger batch of other signals, and
    frame by frame as 23 separate calls."""
    fb = _fb()
    x = _as(_case("speech"), dtype)
    alone, flen = fb(torch.from_numpy(x))
    assert tuple(alone.shape) == (1, 23, 40) and flen.cpu().tolist() == [23]
    others = [_as(_case(k), dtype) for k in ("noise", "tones")]
    pcm, n = _batch([others[0], others[1][:1234], x, others[0][:3000], others[1][:399]], dtype)
    wide, _ = fb(pcm, n, out=torch.empty(5, 40, 40, device="cuda"))
    assert torch.equal(wide[2, :23], alone[0]) and not bool(wide[2, 23:].any())
    for k in range(23):
        one, _ = fb(torch.from_numpy(x[160 * k:160 * k + 400].copy()))
        assert torch.equal(one[0, 0], alone[0, k]), k
    if dtype == "float32":                                   # and the same bits from int16 and float32 input
        assert torch.equal(fb(torch.from_numpy(np.round(x).astype(np.int16)))[0], fb(torch.from_numpy(np.round(x).astype(np.float32)))[0])


# ---------------------------------------------------------------- into the engine

def _speech(n, seed):
    rng = np.random.default_rng(seed)
    x = (np.cumsum(rng.normal(0, 1, n)) * 50 % 20000) - 10000 + rng.normal(0, 200, n)
    return torch.from_numpy(np.round(np.clip(x, -32768, 32767)).astype(np.int16))


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
    """Samples through StreamPool(audio=True) in uneven pieces: the frames in the encoder's window buffer at every chunk are
    the frames the feature-mode pool is given when fed Fbank(whole signal), and the n-best is the same; two sessions that
    start at different steps give what each gives alone."""
    from m3asr.decode import StreamingCtcDecoder
    from m3asr.serve import StreamPool
    eng, B = causal_engine, 2
    fb = _fb(eng.cfg.input_dim)
    xa, xb = _speech(16000, 5), _speech(9000, 6)
    fa, fb_ = (fb(x)[0][0].cpu() for x in (xa, xb))
    Tp = 64

    def pools():
        ta = _Tap(StreamingCtcDecoder(eng.streaming(B, Tp, independent=True), beam=4))
        tf = _Tap(StreamingCtcDecoder(eng.streaming(B, Tp, independent=True), beam=4))
        return ta, StreamPool(ta, audio=True), tf, StreamPool(tf)

    ta, audio, tf, feats = pools()
    got = _drive(audio, audio.push_audio, [(0, xa)], [1, 159, 160, 401, 5000, 777])
    want = _drive(feats, feats.push, [(0, fa)], [50])
    assert len(ta.seen) == len(tf.seen) == 6 and got == want and len(want[0]) > 1
    for (f, v), (g, w) in zip(ta.seen, tf.seen):
        assert torch.equal(v, w) and torch.equal(f, g)
    assert ta.seen[-1][1].tolist()[0] < 19                                            # the short last window ran too
    # two sessions, the second one three steps late: each as if alone
    alone_b = _drive(feats, feats.push, [(0, fa[:0]), (0, fb_)], [50])[1]              # alone, in slot 1 (an empty session holds slot 0)
    ta, audio, _, _ = pools()
    both = _drive(audio, audio.push_audio, [(0, xa), (3, xb)], [2000, 333, 1280])
    assert both[0] == want[0] and both[1] == alone_b and both[0] != both[1]


def test_infer_audio_equals_infer_on_fbank(golden):
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg, _ = golden("tiny")
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=3))
    pcm = torch.stack([_speech(8000, 7), _speech(8000, 8)])
    n = torch.tensor([8000, 5555])
    feat, flen = _fb(cfg.input_dim)(pcm, n)
    assert tuple(feat.shape) == (2, 48, cfg.input_dim) and flen.cpu().tolist() == [48, 33]
    want = eng.infer(feat, flen).cpu().clone()
    got = eng.infer_audio(pcm, n).cpu().clone()
    assert torch.equal(got, want) and float(want.abs().max()) > 0
    assert torch.equal(eng.infer_audio(pcm.float().cuda(), n).cpu(), want)             # float32 samples on the device


def test_cli_wav(golden, tmp_path):
    """infer.py -w on a 0.5 s wav prints the same output shape and sum as -i on the saved features (a fresh child each)."""
    from m3asr.plan import pack_weights, save_plan
    from m3asr.weights import make_weights
    cfg, _ = golden("tiny")
    plan, wav, npy = (str(tmp_path / k) for k in ("m.plan", "a.wav", "feat.npy"))
    save_plan(plan, cfg, pack_weights(make_weights(cfg, seed=3), cfg))
    x = _speech(8000, 9)
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(x.numpy().astype("<i2").tobytes())
    np.save(npy, _fb(cfg.input_dim)(x)[0].cpu().numpy())

    def run(*src):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "-p", plan, *src], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.startswith("outputs.shape:") or ln.startswith("outputs.sum:")]

    a, b = run("-w", wav), run("-i", npy)
    assert len(a) == 2 and a == b and a[0].startswith("outputs.shape:(1, 11,"), (a, b)
