#!/usr/bin/env python3
"""The add-deltas launch (m3_add_deltas, csrc/deltas.hip) and the subsamplers' first conv with three input channels
(conv1_relu_kernel<3>) against one input channel at equal row width, timed inside a hipGraph.

  python tools/bench_deltas.py [--bins 40] [--order 2] [--window 2] [--channels 512] [--launches 50] [--replays 20]

Shapes: 1 x 206 frames and 16 x 500 frames.  Per case one JSON line: microseconds per launch = the median over --replays
replays of a captured graph of --launches back-to-back launches on one stream, divided by --launches (so launch latency is
the graph's, not the host's).  The deltas case is the in-place form on rows of (order + 1) * bins columns, as DeltaFbank runs
it; conv1 reads those rows once as one image of idim bins (in_ch = 1) and once as in_ch = 3 images of idim / 3 bins.
The operands stay in cache between launches: these are the numbers of a launch in a warm forward, not HBM rates.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import torch

from m3asr import ops
from m3asr.frontend import add_deltas


def graph_us(fn, launches, replays):
    """us per call of fn inside a captured graph of `launches` calls; median over `replays` replays"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn()
        times = []
        for _ in range(replays + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            g.replay()
            e1.record(s)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
    return statistics.median(times[2:]), min(times[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=40)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--replays", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_deltas needs a GPU"
    idim, C = (a.order + 1) * a.bins, a.channels
    for B, T in ((1, 206), (16, 500)):
        feat = torch.randn(B, T, idim, device="cuda")
        n = torch.full((B,), T, dtype=torch.int32, device="cuda")
        med, best = graph_us(lambda: add_deltas(feat, n, a.order, a.window, out=feat, bins=a.bins), a.launches, a.replays)
        moved = B * T * idim * 4                               # static columns read, delta columns written
        print(json.dumps({"metric": "add_deltas in place, %d x %d frames, %d bins, order %d window %d" % (B, T, a.bins, a.order, a.window),
                          "us_per_launch": round(med, 2), "us_best": round(best, 2), "bytes_moved": moved,
                          "finite": bool(torch.isfinite(feat).all())}), flush=True)
        for in_ch in (1, 3):
            w9c = torch.randn(in_ch * 9, C, device="cuda") / 3
            bias = torch.randn(C, device="cuda")
            out = ops.subsample_conv1_ch(feat, w9c, bias, in_ch)
            med, best = graph_us(lambda: ops.subsample_conv1_ch(feat, w9c, bias, in_ch, out=out), a.launches, a.replays)
            print(json.dumps({"metric": "conv1 in_ch %d, %d x %d frames, idim %d, C %d" % (in_ch, B, T, idim, C),
                              "us_per_launch": round(med, 2), "us_best": round(best, 2), "out_shape": list(out.shape),
                              "flops": 2 * 9 * in_ch * out.numel(), "finite": bool(torch.isfinite(out).all())}), flush=True)


if __name__ == "__main__":
    main()
