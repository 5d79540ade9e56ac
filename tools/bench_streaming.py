#!/usr/bin/env python3
"""Chunk-by-chunk decoding (m3_engine_forward_chunk) timed: latency of one chunk step and the real-time factor it implies.

  python tools/bench_streaming.py [--chunk 16] [--left-chunks 4] [--batch 1] [--weight-dtype f32] [--seconds 20] [--beam N]
                                  [--independent [--stagger N]] [--audio] [--lm [N_NGRAMS]] [--rescore]

18L x 32e encoder with causal conv modules in both encoders, static_chunk_size = chunk (output frames; one chunk = 4 x chunk
input frames of 10 ms), synthetic weights and features.  Every step after the first is a hipGraph replay (the chunk counter
lives on the device).  Prints one JSON line: ms per chunk (p50 / p99 over all steps, hipEvent pairs on the engine stream),
audio seconds per chunk, real-time factor = compute time / audio time, streams one GPU could serve in real time.
--beam N (> 0): also time the CTC decode of every chunk (StreamingCtcDecoder: top-k + prefix beam advance + streaming greedy,
on the engine stream behind the chunk forward) and add "decode_ms_per_chunk" to the line.
--context N (with --beam): the beam search of every stream is biased by one graph of N random phrases (m3asr.context).
--lm [N] (with --beam): after the plain pass the same chunks are decoded again with a synthetic trigram LM of about N n-grams
(default 100000; tools/lm_synth.py) fused into the beam search (StreamingCtcDecoder(lm=), with the --context graph if given):
"lm" carries its "decode_ms_per_chunk" next to the plain one and their ratio.
--rescore (with --beam): two-pass decoding (StreamingCtcDecoder(rescorer=)) with a random attention decoder
of 6 blocks (D = the encoder's, F = 2048, 8 heads).  Every timed step also appends the chunk's residual stream to the per-slot
encoder memory: "append_ms_per_chunk" is that launch alone, "ms_per_chunk_with_append" the chunk forward plus it.  Afterwards
stream 0 is decoded for 125 output frames and ONE dec.rescore(slots=[0]) call is timed with a host clock around it (gather,
the device-to-host reads, the decoder pass, the result lists): "rescore" carries its ms next to the chunk's.
--independent: slot mode (m3_engine_forward_chunk_slots), every stream with its own position; --stagger N: stream b starts N
steps after stream b - 1 and ends as many steps later (idle slots before and after).  The line then also carries "mode" and
the mean number of live slots per timed step.
--audio: time the same chunks fed SAMPLES as well: per step one pinned int16 window per stream ((4 chunk + 2) * 160 + 400
samples) is uploaded and the log-Mel front end (m3asr.frontend.Fbank, one launch) writes the encoder's window buffer before
the chunk runs.  Adds "audio_ms_per_chunk" (upload + front end + chunk) next to the feature-fed "ms_per_chunk", and
"frontend_ms_per_chunk" (upload + front end alone).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr import ops
from m3asr.config import EncoderConfig
from m3asr.engine import Engine
from m3asr.weights import make_weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--left-chunks", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--weight-dtype", default="f32")
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--seconds", type=float, default=20.0, help="audio per stream")
    ap.add_argument("--beam", type=int, default=0, help="> 0: decode every chunk with a prefix beam search of this width")
    ap.add_argument("--context", type=int, default=None, metavar="N_PHRASES", help="with --beam: bias the beam search by N phrases")
    ap.add_argument("--lm", type=int, nargs="?", const=100000, default=None, metavar="N_NGRAMS",
                    help="with --beam: decode the chunks again with an n-gram LM fused into the beam search")
    ap.add_argument("--independent", action="store_true", help="slot mode: every stream has its own chunk counter")
    ap.add_argument("--stagger", type=int, default=0, help="slot mode: stream b starts this many steps after stream b - 1")
    ap.add_argument("--audio", action="store_true", help="also time the chunks fed samples through the log-Mel front end")
    ap.add_argument("--rescore", action="store_true", help="with --beam: keep the encoder memory per slot and time one rescoring call")
    args = ap.parse_args()
    if args.stagger and not args.independent:
        ap.error("--stagger needs --independent")
    if args.rescore and args.beam <= 0:
        ap.error("--rescore needs --beam")
    cfg = EncoderConfig(num_blocks=args.layers, causal=True, embed_causal=True, static_chunk_size=args.chunk,
                        num_decoding_left_chunks=args.left_chunks, weight_dtype=args.weight_dtype)
    w = make_weights(cfg, seed=0)
    eng = Engine.from_state_dict(cfg, w, packed_rows=False)
    n_chunks = max(4, int(args.seconds * 100 / (4 * args.chunk)))
    st = eng.streaming(args.batch, n_chunks * args.chunk, independent=args.independent)
    n_steps = n_chunks + args.stagger * (args.batch - 1)          # every stream decodes n_chunks chunks
    starts = torch.arange(args.batch) * args.stagger
    rng = np.random.default_rng(1234)
    win = torch.from_numpy(rng.random((args.batch, st.window, cfg.input_dim), dtype=np.float32)).to(eng.device)
    valid = torch.full((args.batch,), st.window, dtype=torch.int32, device=eng.device)
    dec = None
    if args.beam > 0:
        from m3asr.decode import StreamingCtcDecoder
        ctx = None
        if args.context is not None:
            from m3asr.context import ContextGraph, ContextSet
            prng, phrases = np.random.default_rng(0), set()
            while len(phrases) < args.context:
                phrases.add(tuple(int(t) for t in prng.integers(1, cfg.output_dim, int(prng.integers(2, 7)))))
            ctx = ContextSet([ContextGraph([list(p) for p in sorted(phrases)], cfg.output_dim)], device=eng.device)
        rescorer = None
        if args.rescore:
            from m3asr.config import DecoderConfig
            from m3asr.plan import pack_decoder
            from m3asr.rescore import AttentionRescorer
            from m3asr.weights import make_decoder_weights
            dcfg = DecoderConfig(vocab=cfg.output_dim, dim=cfg.attention_dim, heads=8, linear_units=2048, num_blocks=6)
            sd = dict(make_decoder_weights(dcfg, seed=0))
            sd.update({n: w[n] for n in ("after_norm.weight", "after_norm.bias")})
            rescorer = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, eng.device)
        dec = StreamingCtcDecoder(st, args.beam, context=ctx, rescorer=rescorer)
        n_out = torch.full((args.batch,), args.chunk, dtype=torch.int32, device=eng.device)
    times, dtimes, mtimes, live = [], [], [], []
    mem_x = None
    for rep in range(3):
        if dec is not None:
            dec.reset(graph_ids=None if dec.context is None else [0] * args.batch)
        else:
            st.reset()
        for n in range(n_steps):
            if args.stagger:
                on = (starts <= n) & (n < starts + n_chunks)
                valid = (on.to(torch.int32) * st.window).to(eng.device)
                if dec is not None:
                    n_out = (on.to(torch.int32) * args.chunk).to(eng.device)
                if rep > 0:
                    live.append(int(on.sum()))
            elif rep > 0:
                live.append(args.batch)
            e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
            e0.record(eng.stream)
            st.step(win, valid)
            e1.record(eng.stream)
            if dec is not None:
                with torch.cuda.stream(eng.stream):
                    dec.beam.advance(st.logits, n_out, eng.stream)
                    ops.ctc_greedy_stream_advance(dec.gdesc, dec.gstate, st.logits, n_out, dec.frame_ids)
            e2.record(eng.stream)
            if args.rescore:
                if mem_x is None:
                    mem_x = st.buffer("x").view(-1, cfg.attention_dim)
                with torch.cuda.stream(eng.stream):
                    ops.aed_memory_append(dec.mdesc, dec.mstate, mem_x, n_out)
            e3.record(eng.stream)
            e3.synchronize()
            if rep > 0:
                times.append(e0.elapsed_time(e1))
                dtimes.append(e1.elapsed_time(e2))
                mtimes.append(e2.elapsed_time(e3))
    t = np.sort(np.array(times))
    audio_s = 4 * args.chunk * 0.01
    p50 = float(np.median(t))
    out = {"metric": "streaming chunk latency, %dL x %de %s, chunk %d frames (%.2f s of audio), %d left chunks, batch %d" % (
               cfg.num_blocks, cfg.num_experts, args.weight_dtype, args.chunk, audio_s, args.left_chunks, args.batch),
           "ms_per_chunk": {"p50": round(p50, 4), "p99": round(float(t[int(0.99 * (len(t) - 1))]), 4), "min": round(float(t[0]), 4), "n": len(t)},
           "kernels_per_chunk": eng.num_kernels(), "audio_s_per_chunk": audio_s,
           "real_time_factor": round(p50 * 1e-3 / audio_s, 5),
           "streams_in_real_time_one_context": int(args.batch * audio_s / (p50 * 1e-3)),
           "state_MB": round(st.state.numel() / 2 ** 20, 1), "graph_captures": eng.num_captures(), "data": "synthetic",
           "mode": "slots" if args.independent else "lockstep", "mean_live_slots": round(float(np.mean(live)), 3)}
    if args.stagger:
        out["stagger_steps"] = args.stagger
    if args.audio:
        from m3asr.frontend import AudioWindowBuffer, Fbank
        fb = Fbank(cfg.input_dim, eng.device)
        n_win = AudioWindowBuffer(args.chunk).window
        host = torch.from_numpy(rng.integers(-3000, 3000, (args.batch, n_win), dtype=np.int16)).pin_memory()
        pcm = torch.zeros(args.batch, n_win, dtype=torch.int16, device=eng.device)
        n_real = torch.full((args.batch,), n_win, dtype=torch.int32, device=eng.device)
        flen = torch.zeros(args.batch, dtype=torch.int32, device=eng.device)
        full = torch.full((args.batch,), st.window, dtype=torch.int32, device=eng.device)
        atimes, ftimes = [], []
        for rep in range(3):
            st.reset()
            for n in range(n_chunks):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record(eng.stream)
                with torch.cuda.stream(eng.stream):
                    pcm.copy_(host, non_blocking=True)
                fb(pcm, n_real, out=st.feat, out_len=flen, stream=eng.stream)
                e1.record(eng.stream)
                st.step(st.feat, full)
                e2.record(eng.stream)
                e2.synchronize()
                if rep > 0:
                    ftimes.append(e0.elapsed_time(e1))
                    atimes.append(e0.elapsed_time(e2))
        a, f = np.sort(np.array(atimes)), np.sort(np.array(ftimes))
        out["audio_ms_per_chunk"] = {"p50": round(float(np.median(a)), 4), "p99": round(float(a[int(0.99 * (len(a) - 1))]), 4),
                                     "min": round(float(a[0]), 4), "n": len(a)}
        out["frontend_ms_per_chunk"] = {"p50": round(float(np.median(f)), 4), "min": round(float(f[0]), 4),
                                        "samples_per_window": n_win}
    if dec is not None:
        d = np.sort(np.array(dtimes))
        if dec.context is not None:
            out["context_phrases"] = args.context
        out["decode_ms_per_chunk"] = {"beam": args.beam, "p50": round(float(np.median(d)), 4),
                                      "p99": round(float(d[int(0.99 * (len(d) - 1))]), 4), "min": round(float(d[0]), 4)}
    if args.rescore:
        import time
        m = np.array(mtimes)
        both = np.array(times) + m
        out["append_ms_per_chunk"] = {"p50": round(float(np.median(m)), 4), "p99": round(float(np.sort(m)[int(0.99 * (len(m) - 1))]), 4),
                                      "min": round(float(m.min()), 4)}
        out["ms_per_chunk_with_append"] = {"p50": round(float(np.median(both)), 4), "min": round(float(both.min()), 4)}
        out["memory_state_MB"] = round(dec.mstate.numel() / 2 ** 20, 1)
        # endpoint latency: stream 0 after 125 output frames, one rescoring call end to end
        frames, per = 125, []
        dec.reset(graph_ids=None if dec.context is None else [0] * args.batch)
        full = torch.full((args.batch,), st.window, dtype=torch.int32, device=eng.device)
        for n in range(-(-frames // args.chunk)):
            cnt = torch.full((args.batch,), min(args.chunk, frames - n * args.chunk), dtype=torch.int32)
            dec.step(win, full, cnt)
        eng.stream.synchronize()
        for rep in range(12):
            t0 = time.perf_counter()
            res = dec.rescore(slots=[0], detail=True)
            eng.stream.synchronize()
            if rep >= 2:
                per.append((time.perf_counter() - t0) * 1e3)
        hyps = res[0][1]
        out["rescore"] = {"ms_per_call": {"p50": round(float(np.median(per)), 3), "min": round(min(per), 3), "max": round(max(per), 3),
                                          "n": len(per)},
                          "memory_frames": int(dec.memory_lengths()[0]), "hypotheses": len(hyps),
                          "decoder_rows": sum(len(h[0]) + 1 for h in hyps), "decoder_blocks": rescorer.cfg.num_blocks,
                          "dim": rescorer.cfg.dim, "vocab": rescorer.cfg.vocab, "beam": args.beam,
                          "chunk_ms_p50": out["ms_per_chunk"]["p50"]}
    if dec is not None and args.lm is not None:
        from lm_synth import synthetic_lm
        from m3asr.decode import StreamingCtcDecoder
        lm = synthetic_lm(args.lm, cfg.output_dim).to(eng.device)
        fdec = StreamingCtcDecoder(st, args.beam, context=dec.context, lm=lm)
        full_out = torch.full((args.batch,), args.chunk, dtype=torch.int32, device=eng.device)
        ftimes = []
        for rep in range(3):
            fdec.reset(graph_ids=None if fdec.context is None else [0] * args.batch)
            for n in range(n_chunks):
                e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                st.step(win, torch.full((args.batch,), st.window, dtype=torch.int32, device=eng.device))
                e1.record(eng.stream)
                with torch.cuda.stream(eng.stream):
                    fdec.beam.advance(st.logits, full_out, eng.stream)
                    ops.ctc_greedy_stream_advance(fdec.gdesc, fdec.gstate, st.logits, full_out, fdec.frame_ids)
                e2.record(eng.stream)
                e2.synchronize()
                if rep > 0:
                    ftimes.append(e1.elapsed_time(e2))
        f = np.sort(np.array(ftimes))
        out["lm"] = {"n_grams": lm.n_grams, "states": lm.n_states, "arcs": lm.n_arcs,
                     "decode_ms_per_chunk": {"p50": round(float(np.median(f)), 4), "p99": round(float(f[int(0.99 * (len(f) - 1))]), 4),
                                             "min": round(float(f[0]), 4)},
                     "p50_over_plain": round(float(np.median(f)) / out["decode_ms_per_chunk"]["p50"], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
