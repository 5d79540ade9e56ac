#!/usr/bin/env python3
"""The log-Mel front end alone (m3_fbank, csrc/fbank.hip), timed: one launch on a (B, N) batch of samples.

  python tools/bench_fbank.py [--batch 16] [--samples 80000] [--bins 40] [--dtype int16] [--iters 50]

Defaults: 16 x 5 s, the longest case of BASELINE configs[2]; `--batch 8 --samples 10960` is one streaming window of 8 slots
at chunk 16.  Prints one JSON line (hipEvent time per launch, p50 / min).  For the kernel's own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fbank.py ...` and read fbank_kernel's row.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr.frontend import Fbank, num_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=80000)
    ap.add_argument("--bins", type=int, default=40)
    ap.add_argument("--dtype", default="int16", choices=["int16", "float32"])
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    fb = Fbank(args.bins, "cuda:0")
    rng = np.random.default_rng(0)
    pcm = torch.from_numpy(rng.integers(-3000, 3000, (args.batch, args.samples), dtype=np.int16)).cuda()
    if args.dtype == "float32":
        pcm = pcm.float()
    T = num_frames(args.samples)
    out = torch.empty(args.batch, T, args.bins, device="cuda")
    flen = torch.zeros(args.batch, dtype=torch.int32, device="cuda")
    n = torch.full((args.batch,), args.samples, dtype=torch.int32, device="cuda")
    times = []
    for i in range(args.iters + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fb(pcm, n, out=out, out_len=flen)
        e1.record()
        e1.synchronize()
        if i >= 5:
            times.append(e0.elapsed_time(e1))
    t = np.sort(np.array(times))
    print(json.dumps({"metric": "log-Mel front end, %d x %d samples %s -> %d x %d frames x %d bins" % (
        args.batch, args.samples, args.dtype, args.batch, T, args.bins),
        "ms_per_launch": {"p50": round(float(np.median(t)), 4), "min": round(float(t[0]), 4), "n": len(t)},
        "frames": args.batch * T, "finite": bool(torch.isfinite(out).all())}))


if __name__ == "__main__":
    main()
