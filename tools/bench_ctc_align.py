#!/usr/bin/env python3
"""CTC forced alignment on the device (m3_ctc_align_emit + m3_ctc_align_path, m3asr.align.CtcAligner) on the batch of
tools/bench_ctc_beam.py: B = 16 utterances of T' = 125 output frames, V = 1434, synthetic logits, the hypotheses being the best
ones of the device prefix beam search on the same logits.

  python tools/bench_ctc_align.py [--batch 16] [--frames 125] [--beam 10] [--reps 20]

align_ms: wall time of one CtcAligner.align() -- upload of the token lists, two launches, the copies back and the host's
unpacking; it ends in a device synchronise (the copies).  emit_ms / path_ms: each launch alone between hipEvents, the median
of --reps after a warm-up; run under `rocprofv3 --kernel-trace --stats`, in a run of its own, for the kernels' own times.
host_ref_ms: the float32 restatement (tests/ctc_align_ref.py, numpy) on the same emissions, one utterance after the other; its
paths are compared with the device's (`same_paths`).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from m3asr import ops
from m3asr.align import CtcAligner
from m3asr.decode import CtcBeamSearch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--vocab", type=int, default=1434)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    B, T, V = args.batch, args.frames, args.vocab
    x = (torch.randn(B, T, V, generator=torch.Generator().manual_seed(0)) * 2.5).cuda()
    lens = [T] * B
    search = CtcBeamSearch(B, args.beam, T)
    search.advance(x, torch.tensor(lens, dtype=torch.int32))
    hyps = [list(u[0][0]) for u in search.nbest()]
    aligner = CtcAligner(V)
    got = aligner.align(x, lens, hyps)                    # warm-up: code objects, the workspace

    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aligner.align(x, lens, hyps)
        walls.append((time.perf_counter() - t0) * 1e3)

    # the two launches alone, on operands that are already on the device
    L = max(len(y) for y in hyps)
    desc = ops.ctc_align_desc(B, V, 0, T, L)
    tok0 = np.concatenate([[0], np.cumsum([len(y) for y in hyps])])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    row0, nf, tokens, d_tok0 = i32([b * T for b in range(B)]), i32(lens), i32([v for y in hyps for v in y]), i32(tok0.tolist())
    ws = torch.empty(ops.ctc_align_workspace_size(desc), dtype=torch.uint8, device="cuda")
    rows = x.reshape(B * T, V)
    emit = ops.ctc_align_emit(desc, rows, row0, nf, tokens, d_tok0)
    out = ops.ctc_align_path(desc, emit, nf, tokens, d_tok0, ws)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts[1:]))

    emit_ms = timed(lambda: ops.ctc_align_emit(desc, rows, row0, nf, tokens, d_tok0, emit=emit))
    path_ms = timed(lambda: ops.ctc_align_path(desc, emit, nf, tokens, d_tok0, ws, out=out))

    import ctc_align_ref
    eh = emit.cpu().numpy()
    t0 = time.perf_counter()
    ref = [ctc_align_ref.align_emit_ref(eh[b, :T, :len(y) + 1], y) for b, y in enumerate(hyps)]
    host_ms = (time.perf_counter() - t0) * 1e3
    same = all(a.ok and a.states == r.state.tolist() and np.float32(a.score) == r.score for a, r in zip(got, ref))
    print(json.dumps({"metric": "CTC forced alignment, B %d x T' %d, V %d, hypotheses of the beam-%d search" % (B, T, V, args.beam),
                      "tokens_per_utterance": {"mean": round(float(np.mean([len(y) for y in hyps])), 1), "max": L},
                      "align_ms": {"p50": round(float(np.median(walls)), 4), "min": round(min(walls), 4), "n": len(walls)},
                      "emit_ms": round(emit_ms, 4), "path_ms": round(path_ms, 4),
                      "emit_bytes_read": B * T * V * 4, "move_table_bytes": int(ws.numel()),
                      "host_ref_ms": round(host_ms, 4), "same_paths": bool(same), "data": "synthetic"}))


if __name__ == "__main__":
    main()
