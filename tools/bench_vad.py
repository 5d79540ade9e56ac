#!/usr/bin/env python3
"""The long-form path on a synthetic recording: the four launches of csrc/vad.hip one by one, then
LongFormTranscriber.transcribe(mode="greedy") against the same audio cut by hand into the same segments and run with one
Engine.infer_audio call per segment -- what a user could do before.

  python tools/bench_vad.py [--minutes 10] [--layers 18] [--experts 32] [--weight-dtype f32] [--launches 20] [--replays 10]
                            [--max-batch 16] [--skip-engine]

The recording: noise bursts of 1 to 25 s (rms 3000) between pauses of 0.4 to 2 s (rms 2), 16 kHz int16, fixed seed.
Per launch one JSON line: microseconds = the median over --replays replays of a captured graph of --launches back-to-back
launches, divided by --launches; the operands stay in cache between launches.  The gather is timed on the first planned batch.
Per end-to-end case one JSON line with the wall time (host clock around work that ends in a stream synchronise) of a first
call, which binds and captures every (B, T) shape it meets, and of a second call on the same object, and the real-time
factor wall / audio of both.  The loop's line also says how its greedy tokens compare with the batched run's: the loop runs
every segment alone (B = 1 kernels, features of the cut audio), so with synthetic weights on noise its arg-max ties fall
differently; `mean_token_similarity` is difflib's ratio per segment, averaged.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr import _lib
from m3asr.frontend import VadConfig, num_frames, segment_gather


def recording(minutes, seed=0):
    rng = np.random.default_rng(seed)
    n = int(minutes * 60 * 16000)
    x = rng.normal(0, 2, n)
    t = int(16000 * 0.5)
    while t < n:
        dur = int(16000 * rng.uniform(1.0, 25.0))
        x[t:t + dur] = rng.normal(0, 3000, min(dur, n - t))
        t += dur + int(16000 * rng.uniform(0.4, 2.0))
    return torch.from_numpy(np.clip(np.round(x), -32768, 32767).astype(np.int16))


def graph_us(fn, launches, replays):
    """us per call of fn inside a captured graph of `launches` calls; median over `replays` replays"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn(s)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn(s)
        times = []
        for _ in range(replays + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            g.replay()
            e1.record(s)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
    return round(statistics.median(times[2:]), 2), round(min(times[2:]), 2)


def launches(pcm, a):
    lib, dev = _lib.load(), "cuda"
    cfg = VadConfig()
    N = pcm.numel() // 8 * 8
    x = pcm[:N].to(dev).view(1, N)
    T = num_frames(N)
    n = torch.tensor([N], dtype=torch.int32, device=dev)
    logE, lens = torch.zeros(1, T, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    flags, thr = torch.zeros(1, T, dtype=torch.uint8, device=dev), torch.zeros(1, device=dev)
    cap = 4096
    seg, cnt = torch.zeros(1, cap, 2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    st = lambda s: C.c_void_p(s.cuda_stream)                                                    # noqa: E731

    def log_energy(s):
        _lib.check(lib.m3_vad_log_energy(x.data_ptr(), 1, N, n.data_ptr(), 1, T, logE.data_ptr(), T, lens.data_ptr(), st(s)), "log_energy")

    def decide(s):
        _lib.check(lib.m3_vad_decide(logE.data_ptr(), T, lens.data_ptr(), 1, T, cfg.energy_threshold, cfg.energy_mean_scale, cfg.context,
                                     cfg.proportion_threshold, flags.data_ptr(), T, thr.data_ptr(), st(s)), "decide")

    def segments(s):
        _lib.check(lib.m3_vad_segments(flags.data_ptr(), T, logE.data_ptr(), T, lens.data_ptr(), 1, T, *cfg.segment_options(),
                                       seg.data_ptr(), cap, cnt.data_ptr(), st(s)), "segments")

    for name, fn, moved in (("m3_vad_log_energy", log_energy, 2 * N + 4 * T), ("m3_vad_decide", decide, 5 * T),
                            ("m3_vad_segments", segments, T)):
        med, best = graph_us(fn, a.launches, a.replays)
        print(json.dumps({"metric": "%s, 1 x %d frames (%.1f min)" % (name, T, N / 960000.0), "us_per_launch": med, "us_best": best,
                          "bytes_moved": moved}), flush=True)
    k = int(cnt.item())
    segs = [tuple(p) for p in seg[0, :k].cpu().tolist()]
    print(json.dumps({"metric": "segments found", "count": k, "voiced_frames": int(flags.sum().item()), "threshold": round(float(thr.item()), 3),
                      "longest": max(e - s for s, e in segs), "shortest": min(e - s for s, e in segs)}), flush=True)
    # the gather of the first planned batch: the four longest segments into (B, 3000, 40)
    order = sorted(segs, key=lambda p: p[0] - p[1])[:4]
    B, T_max, cols = len(order), -(-max(e - s for s, e in order) // 100) * 100, 40
    src = torch.randn(T, cols, device=dev)
    jobs = torch.tensor([(0, s, e) for s, e in order], dtype=torch.int32, device=dev)
    dst, ln = torch.zeros(B, T_max, cols, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    med, best = graph_us(lambda s: segment_gather(src, jobs, dst, ln, stream=s), a.launches, a.replays)
    print(json.dumps({"metric": "m3_segment_gather, %d x %d frames x %d columns" % (B, T_max, cols), "us_per_launch": med, "us_best": best,
                      "bytes_moved": 4 * cols * (sum(e - s for s, e in order) + B * T_max)}), flush=True)
    return segs


def end_to_end(pcm, a):
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.longform import LongFormTranscriber
    from m3asr.weights import make_weights
    cfg = EncoderConfig(num_blocks=a.layers, num_experts=a.experts, weight_dtype=a.weight_dtype)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=0))
    audio_s = pcm.numel() / 16000.0
    what = "%d layers x %d experts %s, %.1f min" % (a.layers, a.experts, a.weight_dtype, audio_s / 60)
    lf = LongFormTranscriber(eng, max_batch=a.max_batch)
    walls, tokens = [], None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = lf.transcribe(pcm, mode="greedy")
        walls.append(time.perf_counter() - t0)
        tokens = [s.tokens for s in out]
    segs = [(s.start_ms // 10, s.end_ms // 10) for s in out]
    plan = lf.plan_batches(segs)
    print(json.dumps({"metric": "transcribe(greedy), " + what, "segments": len(segs), "batches": len(plan),
                      "shapes": len({(len(i), t) for i, t in plan}), "padded_frames": sum(len(i) * t for i, t in plan),
                      "real_frames": sum(e - s for s, e in segs), "captures": eng.num_captures(),
                      "wall_s_first": round(walls[0], 3), "wall_s_second": round(walls[1], 3),
                      "rtf_first": round(walls[0] / audio_s, 5), "rtf_second": round(walls[1] / audio_s, 5)}), flush=True)
    # what a user can do today: the same audio cut by hand into the same segments, one infer_audio call per segment
    loop = eng.clone_context()
    from m3asr import ops
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = []
        for s, e in segs:
            piece = pcm[160 * s: 160 * (e - 1) + 400]                  # the samples of frames [s, e)
            logits = loop.infer_audio(piece)
            _, tok, n_tok = ops.ctc_greedy(logits, None, 0)
            got.append(tok.cpu()[0, :int(n_tok.cpu()[0])].tolist())
        walls.append(time.perf_counter() - t0)
    same = sum(1 for x, y in zip(got, tokens) if x == y)
    import difflib
    alike = [difflib.SequenceMatcher(None, x, y, autojunk=False).ratio() for x, y in zip(got, tokens) if x or y]
    print(json.dumps({"metric": "infer_audio per segment, " + what, "segments": len(segs), "captures": loop.num_captures(),
                      "wall_s_first": round(walls[0], 3), "wall_s_second": round(walls[1], 3),
                      "rtf_first": round(walls[0] / audio_s, 5), "rtf_second": round(walls[1] / audio_s, 5),
                      "segments_with_equal_tokens": same, "tokens": sum(len(x) for x in got),
                      "mean_token_similarity": round(sum(alike) / max(len(alike), 1), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--experts", type=int, default=32)
    ap.add_argument("--weight-dtype", default="f32")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--skip-engine", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vad needs a GPU"
    pcm = recording(a.minutes)
    launches(pcm, a)
    if not a.skip_engine:
        end_to_end(pcm, a)


if __name__ == "__main__":
    main()
