#!/usr/bin/env python3
"""Run an encoder plan -- same command line as the reference's infer.py (:130-137):

    python3 infer.py -p encoder.plan -i feat.npy [-o compare.npy]
    python3 infer.py -p encoder.plan -w speech.wav [-o compare.npy]

feat.npy is (B,T,idim) float32; feat_len = feat.shape[1] for every utterance, as in the reference (infer.py:111-113).
speech.wav (-w, instead of -i) is a 16-bit PCM RIFF file at any sample rate from 1 to 384 kHz with up to 8 channels; unless
it is 16 kHz mono it is first resampled on the device as Kaldi's compute-fbank-feats would (m3asr.frontend.Resampler;
--channel K takes channel K alone, the default is the mean of all channels).  Its log-Mel frames are computed on the device by
the library's Kaldi-style front end (m3asr.frontend.Fbank with the plan's mel bins, and Kaldi's add-deltas behind it for a plan
built with builder.py --add-deltas) and run as a batch of one.
Prints ``time=...ms`` for one forward after a warm-up and the output's shape / sum (reference :81-103).

    python3 infer.py -p encoder.plan -w speech.wav --hotwords words.txt [--hotword-score 3.0] [--beam 10]

words.txt holds one phrase per line as space-separated token ids (the project has no tokenizer).  The output scores are then
searched twice on the device, plain and biased towards the phrases (m3asr.context), and the best hypothesis of each is printed.

    python3 infer.py -p encoder.plan -w speech.wav --lm lm.arpa [--units units.txt] [--lm-weight 0.5] [--length-bonus 0.0]

lm.arpa is an n-gram LM in ARPA format (or an image saved by m3asr.lm.NgramLm.save, *.npy); units.txt maps its words to
token ids (`token id` per line; without it the words are token ids).  The scores are searched plain and with the LM fused into
the ranking (m3asr.lm), together with --hotwords if both are given.  --lm may be given several times, each as PATH or
PATH:SCALE (SCALE multiplies --lm-weight for that LM): the LMs then travel as ONE device image (m3asr.lm.NgramLmSet) and
--lm-use K (default 0) picks the one this run decodes with.  One --lm without a scale and without --lm-use is a plain NgramLm.

    python3 infer.py -p aed.plan -i feat.npy --rescore [--beam 10] [--ctc-weight 0.5] [--reverse-weight 0.3]

Attention rescoring, for a plan built from a joint CTC/attention checkpoint: the batched prefix beam search, then the plan's
attention decoder rescoring every utterance's n-best on the encoder's hidden states (m3asr.rescore).  Prints the first-pass
best and the rescored best hypothesis of each utterance.

    python3 infer.py -p aed.plan -i feat.npy --attention [--beam 10] [--max-steps K] [--ctc-weight W] [--pre-beam P]
                     [--lm lm.arpa [--units units.txt] [--lm-weight A] [--length-bonus B]]

Attention decoding, for such a plan: the attention decoder searches on its own, autoregressively, over the encoder's hidden
states (m3asr.aed_search); --max-steps bounds the tokens per hypothesis (default: the encoder's output frames).  Prints the
best hypothesis of each utterance.  With --ctc-weight W > 0 the search is the one-pass joint CTC/attention search: every candidate
is also scored by its CTC prefix probability on the forward's own CTC output and ranked by (1 - W) att + W ctc; --pre-beam P
candidates per hypothesis go to the CTC scorer.  Both parts are printed.  With --lm the n-gram LM is fused into this search
(not into a prefix beam search): the rank gains lm_weight log P_LM + length_bonus per token, and the LM part is printed too.
With --hotwords words.txt [--hotword-score S] the phrase list also biases this search (it scores the pre-beam, so a
hotword outside a hypothesis's --pre-beam best is not rescued) and the line ends its parts with bonus=; the separate biased
prefix beam search of the list is still run and printed.

    python3 infer.py -p encoder.plan -i feat.npy --timestamps [any of the modes above]

Token times (m3asr.align): after a mode has chosen its best hypothesis -- without a mode, the CTC greedy search's -- the
hypothesis is aligned to the forward's CTC output and one line per token follows an `utt <b> <mode> times:` line,
`<token> <start ms> <end ms> <conf>`, conf being the token's largest posterior inside its span; `no alignment` for a
hypothesis that CTC cannot align.  Without the flag nothing is added to the output.

    python3 infer.py -p encoder.plan -i feat.npy --wfst graph.txt|graph.npy [--words words.txt] [--wfst-beam 16] [--wfst-max-active 7000]
                     [--acoustic-scale 1.0] [--wfst-blank-skip P]

WFST decoding (m3asr.wfst): the CTC output is searched through a decoding graph (TLG) on the device and the words
are printed.  --wfst-blank-skip P keeps frames whose blank posterior is above P from the search (off by default).graph.txt is AT&T text with numeric labels, as `fstprint TLG.fst` writes it (ilabel = token id + 1, 0 = epsilon);
graph.npy an image saved by DecodingGraph.save (tools/make_lexicon_graph.py writes one from a lexicon).  words.txt (`word id`
per line) turns the word ids into words.  With --timestamps every word is followed by the time of its record, `<word> <ms>`.

    python3 infer.py -p encoder.plan -w meeting.wav --vad [--vad-max-segment 3000 ...] [--max-batch 16] [any of the modes above]

Long recordings (m3asr.longform): the engine refuses an utterance whose subsampled length reaches the plan's
positional table (about 200 s), so with --vad the 16 kHz signal is first cut on the device by Kaldi's energy VAD (compute-vad;
--vad-energy-threshold, --vad-energy-mean-scale, --vad-frames-context, --vad-proportion-threshold) and a segmenter whose options
are in 10-ms frames (--vad-min-silence, --vad-min-speech, --vad-pad, --vad-max-segment, --vad-split-search); the segments run
through the engine in batches of at most --max-batch.  One line per segment, `seg <i> <start>-<end> ms <mode>: <tokens>`, in
time order; the mode is greedy, or biased / fused (--hotwords / --lm: the prefix beam search), rescored (--rescore) or
attention (--attention).  With --timestamps every segment is followed by `seg <i> <mode> times:` and its token lines, on
the recording's clock.  Without --vad nothing changes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))

import numpy as np

import trt_helper
from trt_helper import trt


def read_wav(path):
    """16-bit PCM -> ((1, N, channels) int16, sample rate, channels)"""
    import wave
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise SystemExit("%s: need 16 kHz mono 16-bit PCM, got %d Hz, %d channel(s), %d-bit" % (
                path, w.getframerate(), w.getnchannels(), 8 * w.getsampwidth()))
        if not 1 <= w.getnchannels() <= 8:
            raise SystemExit("%s: need 1 to 8 channels, got %d" % (path, w.getnchannels()))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
        return pcm.reshape(1, -1, w.getnchannels()), w.getframerate(), w.getnchannels()


def wav_features(path, channel, cfg, device):
    """The wav's feature frames (1, T, input_dim), computed on the device: log-Mel, with Kaldi's add-deltas behind it when the
    plan's config says the model was trained on delta features; resampled there first unless it is 16 kHz mono."""
    from m3asr._lib import M3Error
    from m3asr.frontend import make_frontend, Resampler
    pcm, rate, channels = read_wav(path)
    if not -1 <= channel < channels:
        raise SystemExit("%s: --channel %d, the file has %d channel(s)" % (path, channel, channels))
    fb = make_frontend(cfg, device)
    if (rate, channels) == (16000, 1):
        return fb(pcm[:, :, 0])[0]
    try:
        samples, n = Resampler(rate, device, channels=channels, channel=channel)(pcm)
    except M3Error as e:
        raise SystemExit("%s: %s" % (path, e))
    return fb(samples, n)[0]


def print_times(scores, device, mode, hyps):
    """--timestamps: `utt <b> <mode> times:` and one `token start_ms end_ms conf` line per token of hyps[b], aligned to the
    forward's CTC output (all T' frames, blank = 0)."""
    import torch
    from m3asr.align import CtcAligner
    x = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    x = x.reshape(-1, x.shape[-2], x.shape[-1])
    B, T, V = x.shape
    for b, a in enumerate(CtcAligner(V, device=device).align(x, [T] * B, hyps)):
        print("utt %d %s times:" % (b, mode))
        if not a.ok:
            print("no alignment")
        for tok, s, e, c in zip(a.tokens, a.start_ms, a.end_ms, a.conf):
            print("%d %d %d %.4f" % (tok, s, e, c))


def greedy_hyps(scores, device):
    """the CTC greedy hypothesis of every utterance (blank = 0, all T' frames)"""
    import torch
    from m3asr import ops
    x = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    x = x.reshape(-1, x.shape[-2], x.shape[-1])
    _, tokens, n_tokens = ops.ctc_greedy(x, None, 0)
    tokens = tokens.cpu()
    return [tokens[b, :n].tolist() for b, n in enumerate(n_tokens.cpu().tolist())]


def print_hotword_search(scores, device, args):
    """Best prefix beam hypothesis of every utterance without and with the hotword list (blank = 0, all T' frames)."""
    import torch
    from m3asr.context import ContextGraph, ContextSet, read_phrases
    from m3asr.decode import CtcBeamSearch
    x = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    x = x.reshape(-1, x.shape[-2], x.shape[-1])
    B, T, V = x.shape
    ctx = ContextSet([ContextGraph(read_phrases(args.hotwords), V, score=args.hotword_score)], device=device)
    lens = torch.full((B,), T, dtype=torch.int32)
    plain = CtcBeamSearch(B, args.beam, T, device=device)
    plain.advance(x, lens)
    biased = CtcBeamSearch(B, args.beam, T, device=device, context=ctx)
    biased.reset(graph_ids=[0] * B)
    biased.advance(x, lens)
    chosen = biased.nbest(detail=True)
    for b, (u, h) in enumerate(zip(plain.nbest(), chosen)):
        print("utt %d plain:  score=%.4f tokens=%s" % (b, u[0][1], " ".join(str(t) for t in u[0][0])))
        print("utt %d biased: score=%.4f bonus=%.4f tokens=%s" % (b, h[0][1], h[0][2], " ".join(str(t) for t in h[0][0])))
    return [list(h[0][0]) for h in chosen]


def load_lm(args, V, device):
    """--lm [--units] [--lm-use]: ARPA files compiled for V tokens, or saved images; validated and uploaded.  One --lm without a
    scale and without --lm-use: (NgramLm, None).  Else (NgramLmSet of all of them, the member --lm-use picks as lm_on)."""
    from m3asr.lm import load_lms
    try:
        lm, lm_on = load_lms(args.lm, args.units, V, args.lm_use)
    except ValueError as e:
        raise SystemExit("--lm / --lm-use: %s" % e)
    return lm.to(device), lm_on


def print_lm_search(scores, device, args):
    """Best prefix beam hypothesis of every utterance without and with the LM (and the hotwords, if given) fused in."""
    import torch
    from m3asr.decode import CtcBeamSearch
    x = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    x = x.reshape(-1, x.shape[-2], x.shape[-1])
    B, T, V = x.shape
    lm, lm_on = load_lm(args, V, device)
    ctx = None
    if args.hotwords:
        from m3asr.context import ContextGraph, ContextSet, read_phrases
        ctx = ContextSet([ContextGraph(read_phrases(args.hotwords), V, score=args.hotword_score)], device=device)
    lens = torch.full((B,), T, dtype=torch.int32)
    plain = CtcBeamSearch(B, args.beam, T, device=device)
    plain.advance(x, lens)
    fused = CtcBeamSearch(B, args.beam, T, device=device, context=ctx, lm=lm, lm_weight=args.lm_weight,
                          length_bonus=args.length_bonus)
    if ctx is not None or lm_on is not None:
        fused.reset(graph_ids=[0] * B if ctx is not None else None, lm_on=None if lm_on is None else [lm_on] * B)
    fused.advance(x, lens)
    chosen = fused.nbest(detail=True)
    for b, (u, h) in enumerate(zip(plain.nbest(), chosen)):
        print("utt %d plain: score=%.4f tokens=%s" % (b, u[0][1], " ".join(str(t) for t in u[0][0])))
        print("utt %d fused: score=%.4f bonus=%.4f lm=%.4f tokens=%s" % (b, h[0][1], h[0][2], h[0][3],
                                                                         " ".join(str(t) for t in h[0][0])))
    return [list(h[0][0]) for h in chosen]


def print_wfst_search(scores, device, args, frame_ms=40):
    """--wfst: the words of every utterance (all T' frames), found by token passing over the decoding graph."""
    import torch
    from m3asr._lib import M3Error
    from m3asr.wfst import DecodingGraph, read_words, wfst_from_logits
    x = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    x = x.reshape(-1, x.shape[-2], x.shape[-1])
    B, T, V = x.shape
    try:
        graph = (DecodingGraph.load(args.wfst) if args.wfst.endswith(".npy") else DecodingGraph.from_fst_text(args.wfst, V)).to(device)
        if graph.vocab_size != V:
            raise ValueError("the graph was built for %d tokens, the plan has %d" % (graph.vocab_size, V))
        names = read_words(args.words) if args.words else {}
        out = wfst_from_logits(x, torch.full((B,), T, dtype=torch.int32), graph, beam=args.wfst_beam, max_active=args.wfst_max_active,
                               acoustic_scale=args.acoustic_scale, blank_skip=args.wfst_blank_skip, detail=True)
    except (ValueError, OSError, M3Error) as e:
        raise SystemExit("--wfst: %s" % e)
    for b, r in enumerate(out):
        words = [names.get(w, str(w)) for w in r["words"]]
        print("utt %d wfst: cost=%.4f final=%d words=%s" % (b, r["cost"], r["reached_final"], " ".join(words)))
        if args.timestamps:
            print("utt %d wfst times:" % b)
            for w, f in zip(words, r["frames"]):
                print("%s %d" % (w, f * frame_ms))


def print_rescore(helper, feat, feat_len, args):
    """Best hypothesis of every utterance after the first pass and after attention rescoring."""
    import torch
    from m3asr.decode import CtcDecoder
    from m3asr.plan import decoder_config_of
    from m3asr.rescore import AttentionRescorer
    rescorer = AttentionRescorer(helper.decoder_packed, decoder_config_of(helper.extra), helper.engine.device)
    dec = CtcDecoder(helper.engine, rescorer=rescorer)
    out = dec.attention_rescoring(torch.from_numpy(feat), torch.from_numpy(feat_len), args.beam, ctc_weight=args.ctc_weight,
                                  reverse_weight=args.reverse_weight, detail=True)
    for b, (best, hyps) in enumerate(out):
        if not hyps:
            print("utt %d: no hypothesis" % b)
            continue
        chosen = next(h for h in hyps if h[0] == best)
        print("utt %d ctc:      prior=%.4f tokens=%s" % (b, hyps[0][1], " ".join(str(t) for t in hyps[0][0])))
        print("utt %d rescored: att=%.4f final=%.4f tokens=%s" % (b, chosen[2], chosen[3], " ".join(str(t) for t in best)))
    return [list(best) for best, _ in out]


def print_attention(helper, feat, feat_len, args):
    """Best hypothesis of every utterance of the attention decoder's own beam search."""
    import torch
    from m3asr.decode import CtcDecoder
    from m3asr.plan import decoder_config_of
    from m3asr.rescore import AttentionRescorer
    rescorer = AttentionRescorer(helper.decoder_packed, decoder_config_of(helper.extra), helper.engine.device)
    dec = CtcDecoder(helper.engine, rescorer=rescorer)
    lm, lm_on = load_lm(args, rescorer.cfg.vocab, helper.engine.device) if args.lm else (None, None)
    ctx = None
    if args.hotwords:                                             # the list also goes into the attention search
        from m3asr.context import ContextGraph, ContextSet, read_phrases
        V = rescorer.cfg.vocab
        ctx = ContextSet([ContextGraph(read_phrases(args.hotwords), V, score=args.hotword_score)], device=helper.engine.device)
    out = dec.attention(torch.from_numpy(feat), torch.from_numpy(feat_len), args.beam, max_steps=args.max_steps, detail=True,
                        ctc_weight=args.ctc_weight, pre_beam=args.pre_beam, lm=lm, lm_weight=args.lm_weight,
                        length_bonus=args.length_bonus, context=ctx, lm_on=lm_on)
    for b, (best, hyps) in enumerate(out):
        chosen = next(h for h in hyps if list(h[0]) == best)
        parts = " att=%.4f ctc=%.4f" % (chosen[3], chosen[4]) if args.ctc_weight > 0 or lm is not None or ctx is not None else ""
        if lm is not None:
            parts += " lm=%.4f" % chosen[5]
        if ctx is not None:                                       # what the key holds; equal to the final credit once finished
            parts += " bonus=%.4f" % chosen[-2]
        print("utt %d attention: score=%.4f%s finished=%d tokens=%s" % (b, chosen[1], parts, chosen[2], " ".join(str(t) for t in best)))
    return [list(best) for best, _ in out]


def print_long_form(helper, args):
    """--vad: the recording cut by the energy VAD, its segments batched through the engine and decoded in the mode asked for"""
    from m3asr._lib import M3Error
    from m3asr.frontend import VadConfig
    from m3asr.longform import LongFormTranscriber
    pcm, rate, channels = read_wav(args.wav_file)
    if not -1 <= args.channel < channels:
        raise SystemExit("%s: --channel %d, the file has %d channel(s)" % (args.wav_file, args.channel, channels))
    dev, kw, rescorer = helper.engine.device, {}, None
    if args.rescore or args.attention:
        from m3asr.plan import decoder_config_of
        from m3asr.rescore import AttentionRescorer
        rescorer = AttentionRescorer(helper.decoder_packed, decoder_config_of(helper.extra), dev)
    V = rescorer.cfg.vocab if rescorer is not None else helper.cfg.output_dim
    lm, lm_on = load_lm(args, V, dev) if args.lm else (None, None)
    ctx = None
    if args.hotwords:
        from m3asr.context import ContextGraph, ContextSet, read_phrases
        ctx = ContextSet([ContextGraph(read_phrases(args.hotwords), V, score=args.hotword_score)], device=dev)
    if args.attention:
        mode, name = "attention", "attention"
        kw = dict(beam_size=args.beam, max_steps=args.max_steps, ctc_weight=args.ctc_weight, pre_beam=args.pre_beam, lm=lm,
                  lm_weight=args.lm_weight, length_bonus=args.length_bonus, context=ctx, lm_on=lm_on)
    elif args.rescore:
        mode, name = "rescore", "rescored"
        kw = dict(beam_size=args.beam, ctc_weight=args.ctc_weight, reverse_weight=args.reverse_weight)
    elif lm is not None or ctx is not None:
        mode, name = "beam", "fused" if lm is not None else "biased"
        kw = dict(beam_size=args.beam, lm=lm, lm_weight=args.lm_weight, length_bonus=args.length_bonus, context=ctx, lm_on=lm_on)
    else:
        mode, name = "greedy", "greedy"
    try:
        vad = VadConfig(args.vad_energy_threshold, args.vad_energy_mean_scale, args.vad_frames_context, args.vad_proportion_threshold,
                        args.vad_min_silence, args.vad_min_speech, args.vad_pad, args.vad_max_segment, args.vad_split_search)
        lf = LongFormTranscriber(helper.engine, vad=vad, max_batch=args.max_batch, rescorer=rescorer)
        segs = lf.transcribe(pcm, sample_rate=rate, channels=channels, channel=args.channel, mode=mode, timestamps=args.timestamps, **kw)
    except (ValueError, M3Error) as e:
        raise SystemExit("%s: %s" % (args.wav_file, e))
    for i, s in enumerate(segs):
        print("seg %d %d-%d ms %s: %s" % (i, s.start_ms, s.end_ms, name, " ".join(str(t) for t in s.tokens)))
        if args.timestamps:
            print("seg %d %s times:" % (i, name))
            if s.times is None:
                print("no alignment")
            for tok, a, b, c in s.times or []:
                print("%d %d %d %.4f" % (tok, a, b, c))


def main(args):
    logger = trt_helper.init_trt_plugin(trt.Logger.INFO, "libm3asr_hip.so")
    helper = trt_helper.InferHelper(args.plan_name, logger)
    if args.vad:
        if not args.wav_file:
            raise SystemExit("--vad cuts a recording: it needs -w, not -i")
        return print_long_form(helper, args)
    if args.wav_file:
        feat = wav_features(args.wav_file, args.channel, helper.cfg, helper.engine.device).cpu().numpy()
    else:
        feat = np.load(args.input_file).astype(np.float32)
    feat_len = np.full((1, feat.shape[0]), feat.shape[1], dtype=np.int32)
    base = [np.load(args.compare_output_file)] if args.compare_output_file else None
    try:
        outputs = helper.infer([feat, feat_len], base)
    except Exception as e:
        if args.wav_file and "exceeds the positional table" in str(e):    # the engine's refusal of an over-long utterance
            raise type(e)("%s  A recording this long has to be cut first: add --vad." % e) from None
        raise
    for o in outputs:
        print("outputs.shape:" + str(o.shape))
        print("outputs.sum:" + str(o.sum()))
        print(o)
    chosen = []                                                   # (mode, best hypothesis per utterance) of every mode that ran
    if args.rescore:
        chosen.append(("rescored", print_rescore(helper, feat, feat_len, args)))
    if args.attention:
        chosen.append(("attention", print_attention(helper, feat, feat_len, args)))
    if args.lm and not args.attention:                            # with --attention the LM goes into the attention search
        chosen.append(("fused", print_lm_search(outputs[0], helper.engine.device, args)))
    elif args.hotwords:
        chosen.append(("biased", print_hotword_search(outputs[0], helper.engine.device, args)))
    if args.wfst:
        print_wfst_search(outputs[0], helper.engine.device, args)
    if args.timestamps and (chosen or not args.wfst):
        for mode, hyps in chosen or [("greedy", greedy_hyps(outputs[0], helper.engine.device))]:
            print_times(outputs[0], helper.engine.device, mode, hyps)
    if base is not None:
        print("compare_output=%s, dtype=%s, shape=%s" % (args.compare_output_file, base[0].dtype, base[0].shape))
        print("output.sum:" + str(base[0].sum()))


if __name__ == "__main__":
    p = argparse.ArgumentParser(description="3M-ASR encoder inference (MI355X)")
    p.add_argument("-p", "--plan_name", required=True, help="The plan file path.")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("-i", "--input_file", help="The input feat.npy file path.")
    src.add_argument("-w", "--wav", dest="wav_file", help="A 16-bit PCM wav file (any rate, up to 8 channels), instead of feat.npy.")
    p.add_argument("--channel", type=int, default=-1, help="-w: take this channel alone (default: the mean of all channels).")
    p.add_argument("-o", "--compare_output_file", required=False, help="The compare output .npy file path.")
    p.add_argument("--hotwords", help="Phrase list: one phrase of space-separated token ids per line.")
    p.add_argument("--hotword-score", type=float, default=3.0, help="Bonus per matched token (log domain).")
    p.add_argument("--beam", type=int, default=10, help="Beam size of the prefix beam searches run with --hotwords / --lm.")
    p.add_argument("--lm", action="append", metavar="PATH[:SCALE]", help="n-gram LM: an ARPA file, or a compiled image (*.npy) saved by "
                   "m3asr.lm.NgramLm.save.  Given several times (each with an optional :SCALE on --lm-weight), the LMs become one LM set.")
    p.add_argument("--lm-use", type=int, default=None, metavar="K", help="Several --lm: the one this run decodes with (default 0).")
    p.add_argument("--units", help="`token id` per line: the ARPA's words as token ids (default: the words are token ids).")
    p.add_argument("--lm-weight", type=float, default=0.5, help="Weight of log P_LM in the ranking.")
    p.add_argument("--length-bonus", type=float, default=0.0, help="Bonus per token of a prefix in the ranking.")
    p.add_argument("--rescore", action="store_true", help="Attention rescoring of the n-best with the plan's AED decoder.")
    p.add_argument("--ctc-weight", type=float, default=0.0, help="--rescore: weight of the first-pass score in the final score.  --attention: above 0, "
                   "joint CTC/attention decoding with this weight on the CTC prefix score.")
    p.add_argument("--reverse-weight", type=float, default=0.0, help="--rescore: weight of the right-to-left decoder.")
    p.add_argument("--attention", action="store_true", help="Attention decoding: the plan's AED decoder searching on its own.")
    p.add_argument("--max-steps", type=int, default=None, help="--attention: the most tokens per hypothesis.")
    p.add_argument("--pre-beam", type=int, default=None, help="--attention --ctc-weight W: candidates per hypothesis that the CTC scorer sees.")
    p.add_argument("--timestamps", action="store_true", help="Token times: align the chosen hypothesis to the CTC output (start / end ms, confidence).")
    p.add_argument("--wfst", metavar="GRAPH", help="WFST decoding: a decoding graph as AT&T text (fstprint) or a saved image (*.npy).")
    p.add_argument("--words", help="--wfst: `word id` per line, to print words instead of word ids.")
    p.add_argument("--wfst-beam", type=float, default=16.0, help="--wfst: the beam, in cost.")
    p.add_argument("--wfst-max-active", type=int, default=7000, help="--wfst: the most tokens expanded per frame.")
    p.add_argument("--acoustic-scale", type=float, default=1.0, help="--wfst: multiplies the log-probabilities.")
    p.add_argument("--wfst-blank-skip", type=float, default=None, metavar="P",
                   help="--wfst: skip frames whose blank posterior is above P, 0 < P < 1 (an approximation, DESIGN.md 40); default off.")
    p.add_argument("--vad", action="store_true", help="-w: cut a long recording on the device (energy VAD + segmenter) and decode its segments in batches.")
    p.add_argument("--vad-energy-threshold", type=float, default=5.0, help="--vad: Kaldi's vad-energy-threshold.")
    p.add_argument("--vad-energy-mean-scale", type=float, default=0.5, help="--vad: Kaldi's vad-energy-mean-scale.")
    p.add_argument("--vad-frames-context", type=int, default=0, help="--vad: Kaldi's vad-frames-context (0 to 32).")
    p.add_argument("--vad-proportion-threshold", type=float, default=0.6, help="--vad: Kaldi's vad-proportion-threshold.")
    p.add_argument("--vad-min-silence", type=int, default=30, help="--vad: a pause shorter than this many 10-ms frames does not cut.")
    p.add_argument("--vad-min-speech", type=int, default=20, help="--vad: a voiced run shorter than this many frames is dropped (at least 7).")
    p.add_argument("--vad-pad", type=int, default=10, help="--vad: frames kept on either side of a run (at most half of --vad-min-silence).")
    p.add_argument("--vad-max-segment", type=int, default=3000, help="--vad: the longest segment in frames; a longer run is cut at its quietest frame.")
    p.add_argument("--vad-split-search", type=int, default=500, help="--vad: frames back from --vad-max-segment in which the quietest frame is looked for.")
    p.add_argument("--max-batch", type=int, default=16, help="--vad: the most segments per engine batch.")
    main(p.parse_args())
