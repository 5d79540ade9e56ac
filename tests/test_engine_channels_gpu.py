"""Encoders whose subsamplers read the feature blocks as image channels (conv_subsample_in_ch) and models trained on delta
features (delta_order), through the engine: the full forward against tests/inch_ref.py (the oracle's blocks behind a
multi-channel subsample), the streaming path, Engine.infer_audio, StreamPool(audio=True), and builder.py -> infer.py -w.

The bounds are the ones the existing fp32 engine tests hold against the oracle (tests/test_engine_gpu.py: rtol 1e-3 on |logit|
plus atol 2e-4) and the chunked-against-full bound of tests/test_streaming_gpu.py; nothing here chooses a new one."""
import dataclasses
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import inch_ref
from test_engine_gpu import ATOL, RTOL
from m3asr import _lib
from m3asr.config import EncoderConfig
from m3asr.engine import Engine
from m3asr.frontend import DeltaFbank, Fbank
from m3asr.weights import make_weights
from oracle.encoder_ref import sub_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(lengths, idim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(len(lengths), max(lengths), idim, generator=g), torch.tensor(lengths, dtype=torch.int32)


def _check(out, want, fl):
    valid = torch.arange(out.shape[1]).view(1, -1) < sub_len(fl.long()).view(-1, 1)
    err = (out - want).abs()[valid]
    bound = (ATOL + RTOL * want.abs())[valid]
    assert tuple(out.shape) == tuple(want.shape)
    assert bool((err <= bound).all()), "max abs err %.3e, max |ref| %.3e" % (float(err.max()), float(want[valid].abs().max()))
    return float(err.max())


@pytest.mark.parametrize("main_ch,embed_ch,lengths", [(3, 3, [40]), (3, 3, [40, 29, 9]), (3, 1, [40]), (3, 1, [40, 29, 9]),
                                                      (1, 3, [40, 29, 9]), (2, 2, [40, 29, 9])])
def test_forward_against_the_reference(main_ch, embed_ch, lengths):
    cfg = EncoderConfig.tiny(input_dim=48, conv_subsample_in_ch=main_ch, embed_conv_subsample_in_ch=embed_ch)
    w = make_weights(cfg, seed=3)
    feat, fl = _inputs(lengths, 48, 11)
    want = inch_ref.encoder_forward(w, cfg, feat, fl)
    eng = Engine.from_state_dict(cfg, w)
    f, l = feat.cuda().contiguous(), fl.view(1, -1).cuda().contiguous()
    eager = eng(f, l).cpu()
    err = _check(eager, want, fl)
    graph = eng.infer(feat, fl).cpu()
    valid = torch.arange(graph.shape[1]).view(1, -1) < sub_len(fl.long()).view(-1, 1)
    assert torch.equal(graph[valid], eager[valid])
    kern = {s["name"]: s["kernel"] for s in eng.stage_info()}
    assert any("conv1" in k for k in kern.values())
    print("in_ch %d / %d, B %d: max abs err %.2e" % (main_ch, embed_ch, len(lengths), err))


def test_a_plan_with_a_bad_first_conv_is_refused():
    cfg = EncoderConfig.tiny(input_dim=48, conv_subsample_in_ch=3)
    w = make_weights(cfg, seed=3)
    from m3asr.plan import pack_weights
    packed = pack_weights(w, cfg)
    bad = dict(packed)
    bad["subsampling.conv.0.weight_9c"] = torch.zeros(4 * 9, cfg.attention_dim)
    with pytest.raises(_lib.M3Error, match="input channels"):
        Engine(cfg, bad, device="cuda:0")
    bad["subsampling.conv.0.weight_9c"] = torch.zeros(9 * cfg.attention_dim + 1)
    with pytest.raises(_lib.M3Error, match="input channels"):
        Engine(cfg, bad, device="cuda:0")
    cfg50 = EncoderConfig.tiny(input_dim=50)                                      # 50 columns are no 3 channels
    bad = pack_weights(make_weights(cfg50, seed=3), cfg50)
    bad["subsampling.conv.0.weight_9c"] = packed["subsampling.conv.0.weight_9c"]
    with pytest.raises(_lib.M3Error, match="multiple"):
        Engine(cfg50, bad, device="cuda:0")


def test_zero_weight_channels_equal_the_one_channel_engine():
    """the in_ch = 3 engine whose channel-1 and channel-2 weights are zero == the in_ch = 1 engine on feat[..., :16]"""
    cfg3 = EncoderConfig.tiny(input_dim=48, conv_subsample_in_ch=3, embed_conv_subsample_in_ch=3)
    cfg1 = EncoderConfig.tiny(input_dim=16)
    w3 = make_weights(cfg3, seed=8)
    w1 = dict(w3)
    for p in ("subsampling.", "embed.subsampling."):
        w3[p + "conv.0.weight"][:, 1:] = 0
        w1[p + "conv.0.weight"] = w3[p + "conv.0.weight"][:, :1].contiguous()
    feat, fl = _inputs([40, 29], 48, 13)
    a = Engine.from_state_dict(cfg3, w3).infer(feat, fl).cpu().clone()
    b = Engine.from_state_dict(cfg1, w1).infer(feat[..., :16].contiguous(), fl).cpu()
    assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_chunked_equals_full_with_channels():
    cfg = EncoderConfig.tiny(input_dim=48, conv_subsample_in_ch=3, embed_conv_subsample_in_ch=3, causal=True, embed_causal=True,
                             static_chunk_size=4, num_decoding_left_chunks=2)
    w = make_weights(cfg, seed=31)
    feat, fl = _inputs([70, 41], 48, 5)
    eng = Engine.from_state_dict(cfg, w, packed_rows=False)
    full = eng(feat.cuda().contiguous(), fl.view(1, -1).cuda().contiguous()).cpu()
    _check(full, inch_ref.encoder_forward(w, cfg, feat, fl), fl)
    Tp = full.shape[1]
    valid = torch.arange(Tp).view(1, -1) < sub_len(fl.long()).view(-1, 1)
    st = eng.streaming(2, Tp)
    for use_graph in (False, True, True):
        got = st.decode(feat, fl, use_graph=use_graph).cpu()
        err = float((got - full).abs()[valid].max())
        assert err <= 2e-5 * float(full.abs()[valid].max()) + 2e-6, (use_graph, err)       # tests/test_streaming_gpu.py's bound


# ---------------------------------------------------------------- delta features into the engine

def _speech(n, seed):
    rng = np.random.default_rng(seed)
    x = (np.cumsum(rng.normal(0, 1, n)) * 50 % 20000) - 10000 + rng.normal(0, 200, n)
    return torch.from_numpy(np.round(np.clip(x, -32768, 32767)).astype(np.int16))


def _delta_cfg(**kw):
    return EncoderConfig.tiny(input_dim=48, delta_order=2, delta_window=2, conv_subsample_in_ch=3, **kw)


def test_infer_audio_computes_the_deltas():
    cfg = _delta_cfg()
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=3))
    pcm, n = torch.stack([_speech(8000, 7), _speech(8000, 8)]), torch.tensor([8000, 5555])
    feat, flen = DeltaFbank(cfg.num_mel_bins, 2, 2)(pcm, n)
    assert tuple(feat.shape) == (2, 48, 48) and flen.cpu().tolist() == [48, 33]
    want = eng.infer(feat, flen).cpu().clone()
    got = eng.infer_audio(pcm, n).cpu().clone()
    assert torch.equal(got, want) and float(want.abs().max()) > 0
    assert isinstance(eng._fbank, DeltaFbank)
    # the deltas matter to this model, and a config without them still builds the plain front end
    static_only = feat.clone()
    static_only[..., 16:] = 0
    assert not torch.equal(eng.infer(static_only, flen).cpu(), want)
    plain = EncoderConfig.tiny()
    e0 = Engine.from_state_dict(plain, make_weights(plain, seed=3))
    e0.infer_audio(pcm, n)
    assert type(e0._fbank) is Fbank
    # at 8 kHz: resample, fbank, deltas
    pcm8 = torch.stack([_speech(4000, 7), _speech(4000, 8)])
    out8 = eng.infer_audio(pcm8, torch.tensor([4000, 2777]), sample_rate=8000).cpu()
    assert tuple(out8.shape) == tuple(want.shape) and float(out8.abs().max()) > 0


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


def _drive(pool, push, x, pieces):
    sid, sent, step = pool.open(), 0, 0
    while True:
        assert step < 300, "schedule does not end"
        if sent < x.shape[0]:
            k = min(pieces[step % len(pieces)], x.shape[0] - sent)
            push(sid, x[sent:sent + k])
            sent += k
            if sent == x.shape[0]:
                pool.end(sid)
        pool.step()
        if sent == x.shape[0] and not pool.pending(sid):
            return pool.close(sid)
        step += 1


@pytest.mark.parametrize("rate", [16000, 8000])
def test_stream_pool_with_deltas_equals_the_feature_pool(rate):
    """1 s through StreamPool(audio=True) on a delta config in uneven pieces: at every chunk the frames in the encoder's window
    buffer are the offline DeltaFbank's, which a feature-mode pool is given, and the n-best is the same"""
    from m3asr.decode import StreamingCtcDecoder
    from m3asr.frontend import Resampler
    from m3asr.serve import StreamPool
    cfg = _delta_cfg(causal=True, embed_causal=True, static_chunk_size=4, num_decoding_left_chunks=2)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=41), packed_rows=False)
    x = _speech(rate, 5)
    fb = DeltaFbank(cfg.num_mel_bins, 2, 2)
    offline = fb(x) if rate == 16000 else fb(*Resampler(rate, "cuda:0")(x.unsqueeze(0)))
    frames = offline[0][0].cpu()
    assert tuple(frames.shape) == (98, 48)
    ta = _Tap(StreamingCtcDecoder(eng.streaming(2, 64, independent=True), beam=4))
    tf = _Tap(StreamingCtcDecoder(eng.streaming(2, 64, independent=True), beam=4))
    audio = StreamPool(ta, audio=True, sample_rate=rate)
    assert audio.context == 4 and isinstance(audio.fbank, DeltaFbank)
    got = _drive(audio, audio.push_audio, x, [1, rate // 100 + 1, rate // 4 + 9, rate // 2])
    feats = StreamPool(tf)
    want = _drive(feats, feats.push, frames, [50])
    assert len(ta.seen) == len(tf.seen) == 6 and got == want
    for (f, v), (g, w) in zip(ta.seen, tf.seen):
        assert torch.equal(v, w) and torch.equal(f, g)
    assert ta.seen[-1][1].tolist()[0] < 19


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_builder_with_deltas_round_trips_through_infer_wav(tmp_path):
    """synthetic checkpoint with conv_subsample_in_ch 3 on 120 columns -> builder.py --add-deltas 2 -> infer.py -w prints what
    -i prints on the DeltaFbank features made in-process from the same samples"""
    from m3asr.plan import load_plan
    d = str(tmp_path)
    _run(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--add-deltas", "2", "--in-ch", "3", "--seed", "4"])
    plan, wav, npy = (os.path.join(d, k) for k in ("m.plan", "a.wav", "feat.npy"))
    _run(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", os.path.join(d, "model.pt"), "-o", plan, "--opt-shape", "2x80",
          "--add-deltas", "2"])
    cfg = load_plan(plan)[0]
    assert (cfg.input_dim, cfg.num_mel_bins, cfg.delta_order, cfg.delta_window) == (120, 40, 2, 2)
    assert (cfg.conv_subsample_in_ch, cfg.embed_conv_subsample_in_ch) == (3, 1)
    x = _speech(8000, 9)
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(x.numpy().astype("<i2").tobytes())
    np.save(npy, DeltaFbank(40, 2, 2)(x)[0].cpu().numpy())

    def lines(out):
        return [ln for ln in out.splitlines() if ln.startswith("outputs.shape:") or ln.startswith("outputs.sum:")]

    a, b = lines(_run(["infer.py", "-p", plan, "-w", wav])), lines(_run(["infer.py", "-p", plan, "-i", npy]))
    assert len(a) == 2 and a == b and a[0].startswith("outputs.shape:(1, 11,"), (a, b)
