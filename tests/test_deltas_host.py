"""Delta features, the host side (no GPU): the library's filter tables against the float64 restatement of Kaldi's
DeltaFeatures (tests/delta_ref.py), the restatement against the other reading of "delta of a delta", the sample window
buffers with context against a brute-force statement of the window rule, and the config fields."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import delta_ref as D
from m3asr import _lib
from m3asr.config import EncoderConfig
from m3asr.frontend import (AudioWindowBuffer, ResampledWindowBuffer, delta_context, delta_tables, num_frames, num_resampled,
                            resample_span)


# ---------------------------------------------------------------- tables

def test_tables_are_the_literal_numbers():
    s = D.scales(2, 2)
    assert np.allclose(s[1], [-.2, -.1, 0, .1, .2], rtol=0, atol=1e-15)
    assert np.allclose(s[2], [.04, .04, .01, -.04, -.1, -.04, .01, .04, .04], rtol=0, atol=1e-15)
    got = delta_tables(2, 2)
    assert [g.dtype for g in got] == [np.float32] * 3 and [g.shape[0] for g in got] == [1, 5, 9]
    for g, lit in zip(got, ([1], [-.2, -.1, 0, .1, .2], [.04, .04, .01, -.04, -.1, -.04, .01, .04, .04])):
        assert np.array_equal(g, np.asarray(lit, dtype=np.float64).astype(np.float32))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("window", [1, 2, 3, 4])
def test_tables_against_the_restatement(order, window):
    """built in float64, rounded ONCE: each entry is the float32 nearest to the float64 restatement's (one ulp of slack for
    the order of the float64 sums)"""
    got, want = delta_tables(order, window), D.scales(order, window)
    assert len(got) == order + 1 and delta_context(order, window) == order * window
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert np.all(np.abs(g.astype(np.float64) - w) <= 2.0 ** -24 * np.abs(w) + 1e-17)
        assert abs(float(g.astype(np.float64).sum())) < 1e-7 or g.shape[0] == 1   # a delta filter has no DC gain


@pytest.mark.parametrize("order,window", [(0, 2), (3, 2), (2, 0), (2, 5), (-1, 1)])
def test_bad_tables_are_refused(order, window):
    with pytest.raises(_lib.M3Error, match="outside"):
        delta_tables(order, window)


def test_the_restatement_is_not_the_iterated_delta():
    """Kaldi clamps the composite filter's taps on the static frames.  A delta of the (replicate padded) delta agrees with
    it in the interior and differs in the first and last `window` frames of the delta-delta block, nowhere else."""
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (20, 3))
    for window in (2, 3):
        kaldi = D.add_deltas(x, 2, window)[0]
        other = D.iterated_replicate(x, 2, window)
        diff = np.abs(kaldi - other).max(axis=1)
        assert np.all(diff[window:-window] < 1e-12)
        assert np.all(diff[:window] > 1e-3) and np.all(diff[-window:] > 1e-3)
        assert np.abs(kaldi[:, :6] - other[:, :6]).max() < 1e-12                # static and first-order blocks are the same


def test_restatement_on_a_ramp():
    """delta of a ramp is its slope, delta-delta 0, away from the edges"""
    x = np.arange(12, dtype=np.float64).reshape(-1, 1) * 3.0
    y = D.add_deltas(x, 2, 2)[0]
    assert np.allclose(y[4:-4, 1], 3.0) and np.allclose(y[4:-4, 2], 0.0) and np.array_equal(y[:, 0], x[:, 0])
    full = D.add_deltas(x, 2, 2)[0]
    part = D.add_deltas(x[1:11], 2, 2, lead=4, n_out=2)[0]                      # frames 5, 6 with real context on both sides
    assert np.allclose(part, full[5:7], rtol=0, atol=1e-12)


# ---------------------------------------------------------------- window buffers

def _signal(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-30000, 30000, n).astype(np.int16))


def _pieces(n, seed):
    rng, out, left = np.random.default_rng(seed), [], n
    while left > 0:
        k = int(min(left, rng.choice([1, 159, 160, 161, 400, 777, 2500, 6000])))
        out.append(k)
        left -= k
    return out


def _run_plain(buf, x, pieces, R, c):
    """push x in pieces, take every window as soon as it is ready -> [(s0, lead, v, first sample, real samples)], checking
    every window against the brute-force rule and the signal."""
    seen, sent = [], 0
    for k in pieces + [0]:
        if k:
            buf.push(x[sent:sent + k])
            sent += k
        else:
            buf.end()
        while True:
            frames = num_frames(sent)
            want = D.window_rule(frames, buf.chunks, c, R, buf.ended)
            assert buf.ready() == (want[3] if want else 0)
            if not want:
                break
            s0, s1, lead, v = want
            win, real = buf.take()
            assert buf.lead == lead and num_frames(real) == s1 - s0 and real <= buf.window == win.shape[0]
            assert torch.equal(win[:real], x[160 * s0:160 * s0 + real]) and not win[real:].any()
            keep = min(160 * max(4 * c * buf.chunks - R, 0), sent)             # what lies left of the next window is dropped
            assert buf.base == keep and buf.buf.shape[0] == sent - keep
            seen.append((s0, lead, v, 160 * s0, real))
    assert buf.drained()
    return seen


@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("R", [0, 4, 6])
def test_audio_window_buffer_with_context(c, R):
    x = _signal(16000 + 37, 1)
    F = num_frames(x.shape[0])
    seen = _run_plain(AudioWindowBuffer(c, context=R), x, _pieces(x.shape[0], 10 * c + R), R, c)
    # window n produces delta frames [4 c n, 4 c n + v): the first 4 c of every window and all of the last tile [0, F) once
    covered = 0
    for n, (s0, lead, v, _, _) in enumerate(seen):
        assert s0 + lead == 4 * c * n == covered and lead == min(R, 4 * c * n)
        covered += 4 * c if n + 1 < len(seen) else v
    assert covered == F or F - covered < 7 + 3                                  # fewer than 7 frames at the end never run
    assert all(v == 4 * c + 3 for _, _, v, _, _ in seen[:-1])
    # the same windows however the samples are cut
    again = _run_plain(AudioWindowBuffer(c, context=R), x, [x.shape[0]], R, c)
    assert again == seen
    if R == 0:                                                                  # exactly the plain buffer: window n = samples [hop n, ..)
        hop, window = 640 * c, (4 * c + 2) * 160 + 400
        assert AudioWindowBuffer(c).window == AudioWindowBuffer(c, context=0).window == window
        assert [(f, r) for _, _, _, f, r in seen[:-1]] == [(hop * n, window) for n in range(len(seen) - 1)]
        assert seen[-1][3:] == (hop * (len(seen) - 1), min(x.shape[0] - hop * (len(seen) - 1), window))


def test_context_delays_a_window_by_R_frames():
    c, R = 1, 4
    need = 160 * (4 * c + 3 + R - 1) + 400                                      # samples of 4 c + 3 + R frames
    buf = AudioWindowBuffer(c, context=R)
    buf.push(_signal(need - 1, 2))
    assert buf.ready() == 0 and AudioWindowBuffer(c).window < buf.window
    buf.push(_signal(1, 3))
    assert buf.ready() == 4 * c + 3
    short = AudioWindowBuffer(c, context=R)
    short.push(_signal(160 * 6 + 400, 4))                                       # 7 frames: no lookahead, but the stream ends
    assert short.ready() == 0
    short.end()
    assert short.ready() == 7
    with pytest.raises(ValueError, match="context"):
        AudioWindowBuffer(c, context=9)


@pytest.mark.parametrize("R", [4, 6])
def test_rebase_starts_a_fresh_stream(R):
    c = 1
    x = _signal(12000, 5)
    a = AudioWindowBuffer(c, context=R)
    a.push(x)
    for _ in range(3):
        a.take()
    a.rebase()
    b = AudioWindowBuffer(c, context=R)
    b.push(x[640 * c * 3:])
    a.end()
    b.end()
    while b.ready():
        assert a.ready() == b.ready()
        (wa, ra), (wb, rb) = a.take(), b.take()
        assert ra == rb and a.lead == b.lead and torch.equal(wa, wb)
    assert a.lead == min(R, 4 * c * (a.chunks - 1)) and a.drained()


@pytest.mark.parametrize("c,R,rate,channels", [(1, 4, 8000, 1), (4, 6, 44100, 2), (1, 0, 8000, 1), (4, 4, 48000, 1)])
def test_resampled_window_buffer_with_context(c, R, rate, channels):
    n = rate + 123
    x = _signal(n * channels, 6).reshape(n, channels)
    buf = AudioWindowBuffer(c, sample_rate=rate, channels=channels, context=R)
    assert isinstance(buf, ResampledWindowBuffer) and buf.context == R
    assert buf.window == (4 * c + 2 + 2 * R) * 160 + 400
    seen, sent, cut = [], 0, False
    for k in _pieces(n, 3) + [0]:
        if k:
            buf.push(x[sent:sent + k])
            sent += k
        else:
            buf.end()
        while True:
            avail = max(num_resampled(sent, rate, flush=buf.ended) - buf.origin, 0)
            want = D.window_rule(num_frames(avail), buf.chunks, c, R, buf.ended)
            assert buf.ready() == (want[3] if want else 0)
            if not want:
                break
            s0, s1, lead, v = want
            base = buf.base
            win, in0, n_in, out0, n_out = buf.take()
            assert buf.lead == lead and out0 == buf.origin + 160 * s0 and num_frames(n_out) == s1 - s0 and n_out <= buf.window
            lo, hi = resample_span(out0, n_out, rate)
            assert in0 == max(lo, base) and in0 + n_in == min(hi, sent) and in0 <= max(lo, 0) and n_in <= buf.span
            assert torch.equal(win[:n_in], x[in0:in0 + n_in]) and not win[n_in:].any()
            seen.append((out0 - buf.origin, lead, v))
            if len(seen) == 2 and not cut:                                      # a cut: the next segment is a fresh stream
                cut = True
                start = buf.origin + 640 * c * buf.chunks
                buf.rebase()
                assert buf.origin == start and buf.chunks == 0
                seen.append("cut")
    assert buf.drained() and "cut" in seen
    after = seen[seen.index("cut") + 1:]
    assert after and after[0][:2] == (0, 0)                                     # no context in front of the cut
    assert all(lead == min(R, 4 * c * i) for i, (_, lead, _) in enumerate(after))


# ---------------------------------------------------------------- config

def test_config_delta_fields():
    cfg = EncoderConfig.tiny(input_dim=48, delta_order=2, delta_window=3)
    assert cfg.num_mel_bins == 16 and EncoderConfig.tiny().num_mel_bins == 40
    assert cfg.sub_freq == ((48 - 1) // 2 - 1) // 2
    back = EncoderConfig.from_json(cfg.to_json())
    assert back == cfg and json.loads(cfg.to_json())["delta_order"] == 2
    for bad in (dict(delta_order=3), dict(delta_order=-1), dict(delta_window=0), dict(delta_window=5),
                dict(input_dim=40, delta_order=2)):
        with pytest.raises(ValueError, match="delta_order|delta_window|input_dim"):
            EncoderConfig.tiny(**bad)


def test_old_headers_load_and_defaults_are_not_serialised():
    """a header written before the fields existed has none of them, and a config that holds the defaults still writes that
    header: byte for byte what it wrote before"""
    cfg = EncoderConfig.tiny()
    d = json.loads(cfg.to_json())
    new = {"conv_subsample_in_ch", "embed_conv_subsample_in_ch", "delta_order", "delta_window"}
    assert not new & set(d) and new <= {f.name for f in dataclasses.fields(cfg)}
    assert EncoderConfig.from_json(json.dumps(d)) == cfg
    assert (cfg.delta_order, cfg.delta_window, cfg.conv_subsample_in_ch, cfg.embed_conv_subsample_in_ch) == (0, 2, 1, 1)


def test_from_reference_conf_keeps_the_loader_and_channel_settings():
    conf = {"attention_dim": 32, "attention_heads": 2, "num_blocks": 2, "embed_conf": {"attention_dim": 32, "attention_heads": 2}}
    cfg = EncoderConfig.from_reference_conf(120, 16, conf, delta_order=2, delta_window=2)
    assert (cfg.input_dim, cfg.num_mel_bins, cfg.delta_order, cfg.delta_window) == (120, 40, 2, 2)
    assert EncoderConfig.from_reference_conf(40, 16, conf).delta_order == 0
    # the subsamplers' input channels are kept, each encoder's own
    both = dict(conf, conv_subsample_in_ch=3, embed_conf=dict(conf["embed_conf"], conv_subsample_in_ch=2))
    cfg = EncoderConfig.from_reference_conf(120, 16, both, delta_order=2)
    assert (cfg.conv_subsample_in_ch, cfg.embed_conv_subsample_in_ch) == (3, 2)
    assert cfg.sub_freq == ((40 - 1) // 2 - 1) // 2 == 9 and cfg.embed_sub_freq == ((60 - 1) // 2 - 1) // 2 == 14
    main = EncoderConfig.from_reference_conf(120, 16, dict(conf, conv_subsample_in_ch=3))
    assert (main.conv_subsample_in_ch, main.embed_conv_subsample_in_ch, main.embed_sub_freq) == (3, 1, 29)
    assert EncoderConfig.from_json(cfg.to_json()) == cfg
    for bad in (dict(conf, conv_subsample_in_ch=4), dict(conf, conv_subsample_in_ch=0),
                dict(conf, embed_conf=dict(conf["embed_conf"], conv_subsample_in_ch=4))):
        with pytest.raises(ValueError, match="outside"):
            EncoderConfig.from_reference_conf(120, 16, bad)
    with pytest.raises(ValueError, match="multiple"):
        EncoderConfig.tiny(input_dim=40, conv_subsample_in_ch=3)
    with pytest.raises(ValueError, match="7 bins"):
        EncoderConfig.tiny(input_dim=18, embed_conv_subsample_in_ch=3)


def test_weights_and_packing_follow_the_channels():
    """make_weights writes (C, in_ch, 3, 3) first convs and Linear widths on idim / in_ch; the plan's repack is
    [in_ch * 9][C] with row ch * 9 + kh * 3 + kw, and for in_ch = 1 the bytes it always was"""
    from m3asr.plan import pack_weights
    from m3asr.weights import make_weights
    cfg = EncoderConfig.tiny(input_dim=48, conv_subsample_in_ch=3, delta_order=2)
    w = make_weights(cfg, seed=1)
    D = cfg.attention_dim
    assert tuple(w["subsampling.conv.0.weight"].shape) == (D, 3, 3, 3) and tuple(w["embed.subsampling.conv.0.weight"].shape) == (D, 1, 3, 3)
    assert tuple(w["subsampling.out.0.weight"].shape) == (D, D * 3) and tuple(w["embed.subsampling.out.0.weight"].shape) == (D, D * 11)
    packed = pack_weights(w, cfg)
    p9 = packed["subsampling.conv.0.weight_9c"]
    assert tuple(p9.shape) == (27, D)
    for ch, kh, kw in ((0, 0, 0), (1, 2, 1), (2, 1, 2)):
        assert torch.equal(p9[ch * 9 + kh * 3 + kw], w["subsampling.conv.0.weight"][:, ch, kh, kw])
    e9 = packed["embed.subsampling.conv.0.weight_9c"]
    assert torch.equal(e9, w["embed.subsampling.conv.0.weight"].reshape(D, 9).t())
