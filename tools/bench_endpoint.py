#!/usr/bin/env python3
"""Endpoint detection timed.

  python tools/bench_endpoint.py --kernel [--batch 16] [--chunk 16] [--k 10] [--calls 200]
      m3_ctc_endpoint_advance alone on synthetic top-k, for a run under `rocprofv3 --kernel-trace --stats` (the kernel's
      time is read from the trace); prints the hipEvent time per call as well.
  python tools/bench_endpoint.py --pool [--chunk 16] [--left-chunks 4] [--layers 18] [--steps 30] [--rounds 5]
      wall time per StreamPool.step() with segment=True against segment=False on the configuration of
      tools/bench_streaming.py (18L x 32e f32, batch 1, beam 10), rounds interleaved in one process.  The rule never fires,
      so the difference is the endpoint launch plus the one sync per step that reads the detector.  "call" is the time the
      caller's thread spends inside step(); "step" is the steady-state time per step (N steps and a final sync, over N).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr import ops
from m3asr.decode import EndpointConfig, StreamingCtcDecoder
from m3asr.serve import StreamPool


def kernel(a):
    rng = np.random.default_rng(0)
    B, c, k = a.batch, a.chunk, a.k
    ep = EndpointConfig()
    desc = ep.desc(B, 0)
    state = torch.empty(ops.ctc_endpoint_state_size(desc), dtype=torch.uint8, device="cuda")
    idx = torch.from_numpy(rng.integers(0, 3, (B, c, k)).astype(np.int32)).cuda()       # a third of the frames are blank
    lp = torch.from_numpy(-rng.random((B, c, k), dtype=np.float32)).cuda()
    nf = torch.full((B,), c, dtype=torch.int32, device="cuda")
    ops.ctc_endpoint_reset(desc, state)
    for _ in range(10):
        ops.ctc_endpoint_advance(desc, state, lp, idx, nf)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.calls):
        if i % 8 == 0:
            ops.ctc_endpoint_reset(desc, state)                                         # keep the streams unlatched
        ops.ctc_endpoint_advance(desc, state, lp, idx, nf)
    e1.record()
    e1.synchronize()
    fired = int((ops.ctc_endpoint_read(desc, state)[:, 5] != 0).sum())
    print(json.dumps({"metric": "m3_ctc_endpoint_advance, B %d x %d frames, k %d" % (B, c, k), "calls": a.calls,
                      "us_per_call_events": round(e0.elapsed_time(e1) * 1e3 / a.calls, 3), "streams_fired_at_end": fired,
                      "data": "synthetic"}))


def pool(a):
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig(num_blocks=a.layers, causal=True, embed_causal=True, static_chunk_size=a.chunk,
                        num_decoding_left_chunks=a.left_chunks)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=0), packed_rows=False)
    never = EndpointConfig(rules=((True, 10 ** 7, 0),))
    feat = torch.from_numpy(np.random.default_rng(1234).random((4 * a.chunk * a.steps + 3, cfg.input_dim), dtype=np.float32))
    pools = {}
    for seg in (False, True):
        dec = StreamingCtcDecoder(eng.streaming(1, a.steps * a.chunk, independent=True), beam=10, endpoint=never if seg else None)
        pools[seg] = StreamPool(dec, segment=seg)
    call, step = {False: [], True: []}, {False: [], True: []}
    for rnd in range(a.rounds + 1):
        for seg in (False, True):
            p = pools[seg]
            sid = p.open()
            p.push(sid, feat)
            eng.stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                t1 = time.perf_counter()
                assert p.step() == [sid]
                if rnd > 0:
                    call[seg].append((time.perf_counter() - t1) * 1e3)
            eng.stream.synchronize()
            if rnd > 0:
                step[seg].append((time.perf_counter() - t0) * 1e3 / a.steps)
            p.close(sid)
    med = lambda v: round(float(np.median(v)), 4)
    out = {"metric": "StreamPool.step() wall time, %dL x %de f32, chunk %d, %d left chunks, batch 1, beam 10" % (
               cfg.num_blocks, cfg.num_experts, a.chunk, a.left_chunks), "steps": a.steps, "rounds": a.rounds}
    for seg in (False, True):
        out["segment=%s" % seg] = {"call_ms": {"p50": med(call[seg]), "min": round(min(call[seg]), 4)},
                                   "step_ms": {"p50": med(step[seg]), "min": round(min(step[seg]), 4)}}
    out["step_ms_difference_p50"] = round(out["segment=True"]["step_ms"]["p50"] - out["segment=False"]["step_ms"]["p50"], 4)
    out["data"] = "synthetic"
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--kernel", action="store_true")
    mode.add_argument("--pool", action="store_true")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--left-chunks", type=int, default=4)
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    kernel(args) if args.kernel else pool(args)
