#!/usr/bin/env python3
"""Attention rescoring timed: 16 utterances x beam 10 at real dimensions (D 512, 4 heads, F 2048, V 1434,
6 blocks; 125 memory frames = 5 s of audio; hypotheses of 12-30 tokens), synthetic weights and n-best.

  python tools/bench_rescore.py [--batch 16] [--beam 10] [--frames 125] [--blocks 6] [--r-blocks 0] [--rounds 10]

"device": wall time of AttentionRescorer.rescore() per call (launches, the one device-to-host read that sizes the packed
rows, and the read of the results), median over the rounds after a warm-up.  "eager": the same contract as tests/aed_ref.py
states it -- every hypothesis on its own, plain torch float32 -- on the same GPU, median of --eager-rounds.  Prints one JSON
line; the two results are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import aed_ref
from m3asr.config import DecoderConfig
from m3asr.plan import pack_decoder
from m3asr.rescore import AttentionRescorer
from m3asr.weights import make_decoder_weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--r-blocks", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--eager-rounds", type=int, default=2)
    a = ap.parse_args()
    dcfg = DecoderConfig(vocab=1434, dim=512, heads=4, linear_units=2048, num_blocks=a.blocks, r_num_blocks=a.r_blocks)
    rw = 0.3 if a.r_blocks > 0 else 0.0
    sd = make_decoder_weights(dcfg, seed=0)
    g = torch.Generator().manual_seed(0)
    sd["after_norm.weight"], sd["after_norm.bias"] = torch.ones(dcfg.dim), torch.zeros(dcfg.dim)
    B, beam, T = a.batch, a.beam, a.frames
    memory = torch.randn(B, T, dcfg.dim, generator=g)
    mem_len = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32)
    lens = torch.randint(12, 31, (B, beam), generator=g)
    toks = torch.full((B, beam, T), -1, dtype=torch.int32)
    for b in range(B):
        for i in range(beam):
            toks[b, i, :lens[b, i]] = torch.randint(0, dcfg.vocab - 1, (int(lens[b, i]),), generator=g).to(torch.int32)
    score = -torch.rand(B, beam, generator=g) * 10
    tensors = tuple(t.cuda() for t in (toks, lens.to(torch.int32), score, torch.full((B,), beam, dtype=torch.int32)))
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    mem_d = memory.cuda()
    out = res.rescore(mem_d, mem_len, tensors, ctc_weight=0.5, reverse_weight=rw)

    sd_d = {k: v.cuda() for k, v in sd.items()}
    nbest = [[(h[0], h[1]) for h in u[1]] for u in out]

    def eager():
        r = aed_ref.rescore(sd_d, dcfg, mem_d, mem_len.tolist(), nbest, 0.5, rw, dtype=torch.float32)
        torch.cuda.synchronize()
        return r

    ref = eager()
    diff = max(abs(h[3] - v) for u, r in zip(out, ref) for h, v in zip(u[1], r["final"]))
    same = sum(int(list(u[0]) == list(nbest[b][r["best"]][0])) for b, (u, r) in enumerate(zip(out, ref)))

    def timed(f, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    timed(lambda: res.rescore(mem_d, mem_len, tensors, ctc_weight=0.5, reverse_weight=rw), 3)
    dev = timed(lambda: res.rescore(mem_d, mem_len, tensors, ctc_weight=0.5, reverse_weight=rw), a.rounds)
    eag = timed(eager, a.eager_rounds)
    rows = int((lens + 1).sum())
    print(json.dumps({"metric": "attention rescoring, %d utterances x beam %d, %d+%d blocks, D 512 / F 2048 / V 1434, %d frames" % (
        B, beam, a.blocks, a.r_blocks, T), "packed_rows": rows, "device_ms_median": round(statistics.median(dev), 3),
        "device_ms_min": round(min(dev), 3), "eager_aed_ref_ms_median": round(statistics.median(eag), 1),
        "max_abs_final_diff": diff, "same_choice": "%d/%d" % (same, B), "data": "synthetic"}))


if __name__ == "__main__":
    main()
