#!/usr/bin/env python3
"""The resampler launch alone (m3_resample, csrc/resample.hip), timed, next to the m3_fbank launch it feeds.

  python tools/bench_resample.py [--batch 16] [--seconds 30] [--iters 200] [--warmup 20] [--bins 40]

Cases: --batch rows x --seconds at 8000, 44100 and 48000 Hz, int16 mono, and 48000 Hz stereo, all to 16 kHz.  Per case one
JSON line: the time per launch (device events around --iters launches after --warmup), the bytes the launch has to move
(input samples read once + float32 output written once) over that time, the share of the 6.3 TB/s a streaming kernel
reaches on this chip, and the time of ONE m3_fbank launch on the resulting samples in the same process.
The launches rotate over enough copies of the operands to exceed the 256 MiB Infinity Cache, so the bytes come from HBM.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr.frontend import Fbank, Resampler, num_frames

HBM_STREAM = 6.3e12           # bytes/s a float4 copy reaches (of 8.0 TB/s peak)
ROTATE_BYTES = 320 << 20


def timed(fn, sets, iters, warmup):
    """ms per call of fn(k), k cycling over the operand sets"""
    for i in range(warmup):
        fn(i % sets)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % sets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bins", type=int, default=40)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample needs a GPU"
    B, fb, rng = args.batch, Fbank(args.bins, "cuda:0"), np.random.default_rng(0)
    for rate, channels in ((8000, 1), (44100, 1), (48000, 1), (48000, 2)):
        rs = Resampler(rate, "cuda:0", channels=channels)
        N = int(rate * args.seconds) // 8 * 8
        N_out = rs.num_samples(N) // 4 * 4
        moved = B * (N * channels * 2 + N_out * 4)
        sets = max(-(-ROTATE_BYTES // moved), 2)
        pcm = [torch.from_numpy(rng.integers(-3000, 3000, (B, N * channels), dtype=np.int16)).cuda() for _ in range(sets)]
        out = [torch.empty(B, N_out, device="cuda") for _ in range(sets)]
        zero = torch.zeros(B, dtype=torch.int64, device="cuda")
        n_in = torch.full((B,), N, dtype=torch.int32, device="cuda")
        n_out = torch.full((B,), N_out, dtype=torch.int32, device="cuda")
        ms = timed(lambda k: rs.launch(pcm[k], zero, n_in, zero, n_out, out[k]), sets, args.iters, args.warmup)
        T = num_frames(N_out)
        feat = torch.empty(B, T, args.bins, device="cuda")
        flen = torch.zeros(B, dtype=torch.int32, device="cuda")
        ms_fb = timed(lambda k: fb(out[k], n_out, out=feat, out_len=flen), sets, args.iters, args.warmup)
        rate_bytes = moved / (ms * 1e-3)
        print(json.dumps({"metric": "resample %d x %.0f s, %d Hz x %d ch int16 -> 16 kHz float32" % (B, args.seconds, rate, channels),
                          "ms_per_launch": round(ms, 4), "bytes_moved": moved, "TB_per_s": round(rate_bytes / 1e12, 3),
                          "share_of_hbm_stream": round(rate_bytes / HBM_STREAM, 3), "hbm_bound_ms": round(moved / HBM_STREAM * 1e3, 4),
                          "fbank_ms_per_launch": round(ms_fb, 4), "operand_sets": sets,
                          "finite": bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(feat).all())}), flush=True)
        del pcm, out


if __name__ == "__main__":
    main()
