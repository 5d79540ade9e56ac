#!/usr/bin/env python3
"""The device prefix beam search (m3_ctc_beam_advance) against the host routine (m3_ctc_prefix_beam_search) on a configs[2]-like
batch: B = 16 utterances of T' = 125 output frames, V = 1434, beam = k = 10, synthetic logits.

  python tools/bench_ctc_beam.py [--batch 16] [--frames 125] [--beam 10] [--chunk 16] [--reps 5] [--context N_PHRASES]
                                 [--lm N_NGRAMS | --lm-image FILE.npy] [--lm-weight 0.5]

--context N: the biased search (m3_ctc_beam_ctx_advance) with one graph of N random phrases of 2..6 tokens (N = 0: an empty
graph, the cost of the biased kernel alone), next to the unbiased one; its host column is m3_ctc_prefix_beam_search_ctx.

--lm N: the fused search (m3_ctc_beam_lm_advance) with a synthetic trigram LM of about N n-grams (tools/lm_synth.py; or
--lm-image: an image saved by m3asr.lm.NgramLm.save), with the --context graph if one is given, next to the plain search: its
figures, their ratio to the plain ones of the same run, the same kernel with lm_on = 0, and m3_ctc_prefix_beam_search_lm.
--lm-set G (with --lm): the same advance over an NgramLmSet of G such LMs (scales 1.0 / 0.5 / 2.0 in turn): every utterance
on member 0, the members cycling over the utterances, and every utterance off.

Device: one advance over all frames, and the same frames in chunks of --chunk (one advance per chunk), timed with hipEvents
(top-k excluded: it is the same launch for both searches); run under `rocprofv3 --kernel-trace --stats` for kernel times.
Host: the 16 host searches one after another (what CtcDecoder.ctc_prefix_beam_search does per utterance), wall time, with
the device top-k and the copy of its pairs excluded.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--vocab", type=int, default=1434)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--context", type=int, default=None, metavar="N_PHRASES")
    ap.add_argument("--lm", type=int, default=None, metavar="N_NGRAMS")
    ap.add_argument("--lm-image", default=None, metavar="FILE.npy")
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--lm-set", type=int, default=0, metavar="G", help="--lm: also time the fused advance over an LM set of G members")
    args = ap.parse_args()
    B, T, V, beam = args.batch, args.frames, args.vocab, args.beam
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, T, V, generator=g) * 2.5).cuda()
    lp, ix = ops.ctc_topk(x, beam)
    nf = torch.full((B,), T, dtype=torch.int32, device="cuda")
    desc = ops.ctc_beam_desc(B, beam, T, 0)
    state = torch.empty(ops.ctc_beam_state_size(desc), dtype=torch.uint8, device="cuda")
    chunks = [(t0, min(args.chunk, T - t0)) for t0 in range(0, T, args.chunk)]
    nfc = [torch.full((B,), c, dtype=torch.int32, device="cuda") for _, c in chunks]
    lpc = [(lp[:, t0:t0 + c].contiguous(), ix[:, t0:t0 + c].contiguous()) for t0, c in chunks]

    def timed(fn, reset=lambda: ops.ctc_beam_reset(desc, state)):
        ts = []
        for _ in range(args.reps + 1):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts[1:]))

    one = timed(lambda: ops.ctc_beam_advance(desc, state, lp, ix, nf))
    per = timed(lambda: [ops.ctc_beam_advance(desc, state, a, b, n) for (a, b), n in zip(lpc, nfc)])
    lph, ixh = lp.cpu().numpy(), ix.cpu().numpy()
    hs = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for b in range(B):
            ops.ctc_prefix_beam_search_host(lph[b], ixh[b], beam, 0)
        hs.append((time.perf_counter() - t0) * 1e3)
    out = {"metric": "CTC prefix beam search, B %d x T' %d, V %d, beam = k = %d" % (B, T, V, beam),
           "device_one_advance_ms": round(one, 4),
           "device_chunked_ms": {"chunk": args.chunk, "advances": len(chunks), "total": round(per, 4),
                                 "per_advance": round(per / len(chunks), 4)},
           "host_routine_ms": round(float(np.median(hs)), 4), "data": "synthetic"}
    cs = None
    if args.context is not None:
        from m3asr.context import ContextGraph, ContextSet
        rng = np.random.default_rng(0)
        phrases = set()
        while len(phrases) < args.context:
            phrases.add(tuple(int(t) for t in rng.integers(1, V, int(rng.integers(2, 7)))))
        cs = ContextSet([ContextGraph([list(p) for p in sorted(phrases)], V)], device="cuda")
        cstate = torch.empty(ops.ctc_beam_ctx_state_size(desc), dtype=torch.uint8, device="cuda")
        go = torch.zeros(B, dtype=torch.int32, device="cuda")
        creset = lambda: ops.ctc_beam_ctx_reset(desc, cstate)
        c_one = timed(lambda: ops.ctc_beam_ctx_advance(desc, cstate, cs.dev, go, lp, ix, nf), creset)
        c_per = timed(lambda: [ops.ctc_beam_ctx_advance(desc, cstate, cs.dev, go, a, b, n) for (a, b), n in zip(lpc, nfc)], creset)
        hs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for b in range(B):
                ops.ctc_prefix_beam_search_ctx_host(lph[b], ixh[b], beam, 0, cs.image, 0)
            hs.append((time.perf_counter() - t0) * 1e3)
        out["context"] = {"phrases": args.context, "states": cs.graphs[0].n_states, "image_bytes": int(cs.image.nbytes),
                          "device_one_advance_ms": round(c_one, 4),
                          "device_chunked_ms": {"total": round(c_per, 4), "per_advance": round(c_per / len(chunks), 4)},
                          "host_routine_ms": round(float(np.median(hs)), 4)}
    if args.lm is not None or args.lm_image:
        from m3asr.lm import NgramLm
        if args.lm_image:
            lm = NgramLm.load(args.lm_image)
        else:
            from lm_synth import synthetic_lm
            lm = synthetic_lm(args.lm, V)
        lm.to("cuda")
        lstate = torch.empty(ops.ctc_beam_lm_state_size(desc), dtype=torch.uint8, device="cuda")
        go = torch.full((B,), 0 if cs is not None else -1, dtype=torch.int32, device="cuda")
        image = None if cs is None else cs.dev
        lreset = lambda: ops.ctc_beam_lm_reset(desc, lstate)
        a, w = args.lm_weight, 0.0
        res = {}
        for name, flag in (("fused", 1), ("lm_off", 0)):
            on = torch.full((B,), flag, dtype=torch.int32, device="cuda")
            l_one = timed(lambda: ops.ctc_beam_lm_advance(desc, lstate, image, go, lm.dev, on, a, w, lp, ix, nf), lreset)
            l_per = timed(lambda: [ops.ctc_beam_lm_advance(desc, lstate, image, go, lm.dev, on, a, w, p, q, n)
                                   for (p, q), n in zip(lpc, nfc)], lreset)
            res[name] = {"device_one_advance_ms": round(l_one, 4),
                         "device_chunked_ms": {"total": round(l_per, 4), "per_advance": round(l_per / len(chunks), 4)},
                         "one_advance_over_plain": round(l_one / one, 3)}
        hs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for b in range(B):
                ops.ctc_prefix_beam_search_lm_host(lph[b], ixh[b], beam, 0, None if cs is None else cs.image, 0, lm.image, a, w)
            hs.append((time.perf_counter() - t0) * 1e3)
        out["lm"] = {"n_grams": lm.n_grams, "order": lm.order, "states": lm.n_states, "arcs": lm.n_arcs,
                     "image_bytes": int(lm.image.nbytes), "weight": a, "with_context": cs is not None, **res,
                     "host_routine_ms": round(float(np.median(hs)), 4)}
        if args.lm_set:                                # the same advance over an LM set of G members
            from lm_synth import synthetic_lm
            from m3asr.lm import NgramLmSet
            G = args.lm_set
            lms = [lm] + [synthetic_lm(args.lm or lm.n_grams or 20000, V, seed=j) for j in range(1, G)]
            lset = NgramLmSet(lms, [(1.0, 0.5, 2.0)[j % 3] for j in range(G)]).to("cuda")
            sres = {}
            for name, flags in (("member0", [1] * B), ("mixed", [1 + b % G for b in range(B)]), ("all_off", [0] * B)):
                on = torch.tensor(flags, dtype=torch.int32, device="cuda")
                sres[name + "_one_advance_ms"] = round(timed(lambda: ops.ctc_beam_lm_advance(desc, lstate, image, go, lset.dev, on, a, w,
                                                                                            lp, ix, nf), lreset), 4)
            out["lm_set"] = {"members": G, "image_bytes": int(lset.image.nbytes), **sres}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
