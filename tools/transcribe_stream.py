#!/usr/bin/env python3
"""Continuous decoding of a wav file as a live service would see it: the samples go into StreamPool(audio=True, segment=True)
in 100 ms pieces, the device-side endpoint detector cuts the session into utterances, and every finished segment is printed
as soon as the step that ended it returns:

    python tools/transcribe_stream.py -p encoder.plan -w speech.wav [--hotwords words.txt] [--lm lm.arpa] [--beam 10]
                                      [--blank-threshold 0.8] [--rule must_decoded,trailing_ms,length_ms ...]
                                      [--rescore [--ctc-weight 0.5] [--reverse-weight 0.0]]
                                      [--timestamps]

    <start ms>-<end ms> rule <r>: <token ids of the best hypothesis>
    <start ms>-<end ms> rule <r> rescored: att=<a> final=<f> tokens=<token ids the attention decoder chose>      (--rescore)

    <token> <start ms> <end ms> <conf>      one line per token of the segment's final best hypothesis                    (--timestamps)

--timestamps: token times in session time (StreamPool(timestamps=True)): the decoder keeps every session's logits
on the device and aligns a segment's final best hypothesis -- the rescored one with --rescore -- when its utterance ends.
`no alignment` where CTC cannot align it.

--rescore: two-pass decoding.  The plan must come from a joint CTC/attention checkpoint (builder.py packs the decoder when the
checkpoint has one); the decoder keeps every session's encoder memory on the device and the plan's attention decoder rescores
a segment's n-best when its utterance ends (StreamPool(rescore=True)).

The plan must be a streaming one (static_chunk_size > 0, causal conv modules).  speech.wav is 16-bit PCM at any sample rate from 1 to
384 kHz with up to 8 channels: unless it is 16 kHz mono the pool resamples it on the device (StreamPool(sample_rate=,
channels=, channel=)); --channel K takes channel K alone, the default is the mean of all channels.  The
last line (rule 0) is what was still open when the file ended.  --synthetic N pushes N seconds of a generated signal instead
of a file (no plan either: a small random streaming model, with --rescore plus a small random attention decoder), to see
the mechanics on a machine without a model."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr.decode import EndpointConfig, StreamingCtcDecoder
from m3asr.serve import StreamPool

def rescored(best, scores):
    """att=<a> final=<f> tokens=<ids> of the hypothesis the second pass chose (nothing decoded: the scores are missing)"""
    chosen = next((h for h in scores if tuple(h[0]) == tuple(best)), None)
    if chosen is None:
        return "att=nan final=nan tokens="
    return "att=%.4f final=%.4f tokens=%s" % (chosen[2], chosen[3], " ".join(str(t) for t in best))


def read_wav(path):
    """16-bit PCM -> ((N, channels) int16, sample rate, channels)"""
    import wave
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise SystemExit("%s: need 16 kHz mono 16-bit PCM, got %d Hz, %d channel(s), %d-bit" % (
                path, w.getframerate(), w.getnchannels(), 8 * w.getsampwidth()))
        if not 1 <= w.getnchannels() <= 8:
            raise SystemExit("%s: need 1 to 8 channels, got %d" % (path, w.getnchannels()))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
        return pcm.reshape(-1, w.getnchannels()), w.getframerate(), w.getnchannels()


def load_engine(a):
    """-> (engine, AttentionRescorer or None)"""
    if a.synthetic:
        from m3asr.config import DecoderConfig, EncoderConfig
        from m3asr.engine import Engine
        from m3asr.weights import make_decoder_weights, make_weights
        cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=16,
                            num_decoding_left_chunks=2)
        w = make_weights(cfg, seed=0)
        eng, rescorer = Engine.from_state_dict(cfg, w, packed_rows=False), None
        if a.rescore:
            from m3asr.plan import pack_decoder
            from m3asr.rescore import AttentionRescorer
            dcfg = DecoderConfig(vocab=cfg.output_dim, dim=cfg.attention_dim, heads=cfg.attention_heads, linear_units=256,
                                 num_blocks=2, r_num_blocks=1 if a.reverse_weight > 0 else 0)
            sd = dict(make_decoder_weights(dcfg, seed=0))
            sd.update({n: w[n] for n in ("after_norm.weight", "after_norm.bias")})      # the encoder's own final LayerNorm
            rescorer = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, eng.device)
        return eng, rescorer
    import trt_helper
    from trt_helper import trt
    helper = trt_helper.InferHelper(a.plan_name, trt_helper.init_trt_plugin(trt.Logger.INFO, "libm3asr_hip.so"))
    rescorer = None
    if a.rescore:
        from m3asr.plan import decoder_config_of
        from m3asr.rescore import AttentionRescorer
        dcfg = decoder_config_of(helper.extra)
        if dcfg is None:
            raise SystemExit("%s: --rescore needs a plan with an attention decoder (build it from a CTC/attention checkpoint)" % a.plan_name)
        rescorer = AttentionRescorer(helper.decoder_packed, dcfg, helper.engine.device)
    return helper.engine, rescorer


def main(a):
    eng, rescorer = load_engine(a)
    V, kw = eng.cfg.output_dim, {}
    if rescorer is not None:
        kw.update(rescorer=rescorer, ctc_weight=a.ctc_weight, reverse_weight=a.reverse_weight)
    if a.hotwords:
        from m3asr.context import ContextGraph, ContextSet, read_phrases
        kw["context"] = ContextSet([ContextGraph(read_phrases(a.hotwords), V, score=a.hotword_score)], device=eng.device)
    lm_on = None                                                  # several --lm (an LM set): the member --lm-use picks
    if a.lm:
        from m3asr.lm import load_lms
        try:
            lm, lm_on = load_lms(a.lm, a.units, V, a.lm_use)
        except ValueError as e:
            raise SystemExit("--lm / --lm-use: %s" % e)
        kw.update(lm=lm.to(eng.device), lm_weight=a.lm_weight, length_bonus=a.length_bonus)
    if a.timestamps:
        from m3asr.align import CtcAligner
        kw["aligner"] = CtcAligner(V, device=eng.device)
    rules = [tuple(int(v) for v in r.split(",")) for r in a.rule] if a.rule else EndpointConfig().rules
    ep = EndpointConfig(a.blank_threshold, rules)
    bound = ep.length_bound()
    max_frames = a.max_frames or (bound if bound is not None else 2000) + eng.cfg.static_chunk_size
    dec = StreamingCtcDecoder(eng.streaming(1, max_frames, independent=True), beam=a.beam, endpoint=ep, **kw)
    rate, channels = 16000, 1
    if a.synthetic:
        rng = np.random.default_rng(1)
        pcm = np.clip(np.cumsum(rng.normal(0, 1, int(16000 * a.synthetic))) * 50 % 20000 - 10000, -32768, 32767).astype(np.int16)
    else:
        pcm, rate, channels = read_wav(a.wav_file)
        if not -1 <= a.channel < channels:
            raise SystemExit("%s: --channel %d, the file has %d channel(s)" % (a.wav_file, a.channel, channels))
        if (rate, channels) == (16000, 1):
            pcm = pcm[:, 0]
    from m3asr._lib import M3Error
    try:
        pool = StreamPool(dec, audio=True, segment=True, rescore=rescorer is not None, timestamps=a.timestamps, sample_rate=rate,
                          channels=channels, channel=a.channel if channels > 1 else -1)
    except M3Error as e:
        raise SystemExit("%s: %s" % (a.wav_file, e))
    piece = rate // 10                                            # 100 ms of samples
    sid = pool.open(context=0 if a.hotwords else None, lm=lm_on)

    def show_times(times):
        if times is None:
            print("no alignment", flush=True)
        for tok, t0, t1, conf in times or []:
            print("%d %d %d %.4f" % (tok, t0, t1, conf), flush=True)

    def show():
        for s in pool.segments(sid):
            print("%d-%d ms rule %d: %s" % (s.start_ms, s.end_ms, s.rule, " ".join(str(t) for t in s.nbest[0][0])), flush=True)
            if rescorer is not None:
                print("%d-%d ms rule %d rescored: %s" % (s.start_ms, s.end_ms, s.rule, rescored(s.best, s.scores)), flush=True)
            if a.timestamps:
                show_times(s.times)

    for pos in range(0, len(pcm), piece):
        pool.push_audio(sid, torch.from_numpy(pcm[pos:pos + piece].copy()))
        while pool.step():
            show()
    pool.end(sid)
    while pool.step():
        show()
    start = pool.offset_ms(sid)
    rest = pool.close(sid, rescored=rescorer is not None, timed=a.timestamps)
    rest, times = rest if a.timestamps else (rest, None)
    if rescorer is None:
        print("%d- ms rule 0: %s" % (start, " ".join(str(t) for t in rest[0][0]) if rest else ""))
    else:
        best, scores = rest
        print("%d- ms rule 0: %s" % (start, " ".join(str(t) for t in scores[0][0]) if scores else ""))
        print("%d- ms rule 0 rescored: %s" % (start, rescored(best, scores)))
    if a.timestamps:
        show_times(times)
    print("%d engine steps, %.1f s of audio" % (pool.steps, len(pcm) / float(rate)))


if __name__ == "__main__":
    p = argparse.ArgumentParser(description="Continuous streaming decoding of a wav file with endpoint detection (MI355X)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("-w", "--wav", dest="wav_file", help="A 16-bit PCM wav file (any rate, up to 8 channels).")
    p.add_argument("--channel", type=int, default=-1, help="-w: take this channel alone (default: the mean of all channels).")
    src.add_argument("--synthetic", type=float, default=0.0, help="Seconds of a generated signal through a small random model.")
    p.add_argument("-p", "--plan_name", help="The plan file of a streaming encoder (with -w).")
    p.add_argument("--beam", type=int, default=10)
    p.add_argument("--max-frames", type=int, default=0, help="Output frames of the streaming state (default: the length rule + c).")
    p.add_argument("--blank-threshold", type=float, default=0.8)
    p.add_argument("--rule", action="append", help="must_decoded (0/1),min trailing blank ms,min length ms; up to four, in order.")
    p.add_argument("--hotwords", help="Phrase list: one phrase of space-separated token ids per line.")
    p.add_argument("--hotword-score", type=float, default=3.0)
    p.add_argument("--lm", action="append", metavar="PATH[:SCALE]", help="n-gram LM: an ARPA file, or a compiled image (*.npy).  Given "
                   "several times (each with an optional :SCALE on --lm-weight), the LMs become one LM set.")
    p.add_argument("--lm-use", type=int, default=None, metavar="K", help="Several --lm: the one the session decodes with (default 0).")
    p.add_argument("--units", help="`token id` per line: the ARPA's words as token ids.")
    p.add_argument("--lm-weight", type=float, default=0.5)
    p.add_argument("--length-bonus", type=float, default=0.0)
    p.add_argument("--rescore", action="store_true", help="Two passes: the attention decoder rescores every segment's n-best.")
    p.add_argument("--ctc-weight", type=float, default=0.5, help="--rescore: weight of the first-pass score in the final score.")
    p.add_argument("--reverse-weight", type=float, default=0.0, help="--rescore: weight of the right-to-left decoder.")
    p.add_argument("--timestamps", action="store_true", help="Token times of every segment's final best hypothesis, in session time.")
    args = p.parse_args()
    if args.wav_file and not args.plan_name:
        p.error("-w needs -p")
    main(args)
