#!/usr/bin/env python3
"""The WFST search (m3_wfst_search_advance) on a configs[2]-like batch: B = 16 utterances of T' = 125 output frames, V = 1434,
over the from_lexicon graph of --words synthetic words, next to the prefix beam search (CtcBeamSearch, beam 10) on the same
logits in the same process, as context.

  python tools/bench_ctc_wfst.py [--words 1000] [--batch 16] [--frames 125] [--chunk 16] [--beam 16] [--max-active 7000] [--reps 5]
                                  [--blank-skip P]

One advance over all frames, and the same frames in chunks of --chunk (one advance per chunk), timed with hipEvents; the
log-softmax is excluded (one launch, the same for every search).  Run under `rocprofv3 --kernel-trace --stats` for kernel times.
Prints one JSON line."""
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
from m3asr.decode import CtcBeamSearch
from m3asr.wfst import CtcWfstSearch, DecodingGraph


def synthetic_lexicon(n_words, V, seed=0):
    """n_words distinct words of 1..6 tokens over tokens 1..V-1 (Zipf-like first tokens, so that prefixes are shared)."""
    rng = np.random.default_rng(seed)
    seen, lex = set(), {}
    while len(lex) < n_words:
        n = int(rng.integers(1, 7))
        pron = tuple(int(t) for t in 1 + (rng.zipf(1.3, n) - 1) % (V - 1))
        if pron not in seen:
            seen.add(pron)
            lex[len(lex) + 1] = list(pron)
    return lex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--vocab", type=int, default=1434)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--beam", type=float, default=16.0)
    ap.add_argument("--max-active", type=int, default=7000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blank-skip", type=float, default=None, metavar="P",
                    help="also time CtcWfstSearch(blank_skip=P) on the same logits: the share of frames kept, the select launch "
                         "alone, and the total next to the unskipped search's (DESIGN.md 40)")
    args = ap.parse_args()
    B, T, V = args.batch, args.frames, args.vocab
    rng = np.random.default_rng(0)
    lex = synthetic_lexicon(args.words, V)
    costs = {w: float(np.float32(np.log(w + 1.0))) for w in lex}
    graph = DecodingGraph.from_lexicon(lex, V, word_costs=costs).to("cuda")
    # logits peaked on alignments of random word sequences (blanks and repeats in between), noise around them
    x = rng.normal(0.0, 2.5, (B, T, V)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            for tok in lex[int(rng.integers(1, args.words + 1))] + [0]:
                for _ in range(int(rng.integers(1, 3))):
                    if t < T:
                        x[b, t, tok] += 12.0
                        t += 1
    x = torch.from_numpy(x).cuda()
    logp = ops.log_softmax_bias(x)
    nf = torch.full((B,), T, dtype=torch.int32, device="cuda")
    chunks = [(t0, min(args.chunk, T - t0)) for t0 in range(0, T, args.chunk)]
    search = CtcWfstSearch(graph, B, T, beam=args.beam, max_active=args.max_active)

    def timed(fn, reset):
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

    one = timed(lambda: search.advance(logp, nf, log_softmax=False), search.reset)
    res = search.result(detail=True)
    lpc = [(logp[:, t0:t0 + c].contiguous(), torch.full((B,), c, dtype=torch.int32, device="cuda")) for t0, c in chunks]
    per = timed(lambda: [search.advance(a, n, log_softmax=False) for a, n in lpc], search.reset)
    assert [r["words"] for r in search.result(detail=True)] == [r["words"] for r in res], "chunked != one-shot"
    plain = CtcBeamSearch(B, 10, T)
    lp, ix = ops.ctc_topk(x, 10)
    pdesc, pstate = plain.desc, plain.state
    p_one = timed(lambda: ops.ctc_beam_advance(pdesc, pstate, lp, ix, nf), plain.reset)
    out = {"metric": "CTC WFST search, B %d x T' %d, V %d, lexicon graph of %d words, beam %g, max_active %d"
                     % (B, T, V, args.words, args.beam, args.max_active),
           "graph": {"states": graph.n_states, "arcs": graph.n_arcs, "levels": graph.n_levels, "image_bytes": int(graph.image.nbytes)},
           "state_bytes_per_utterance": search.bytes_per_utterance,
           "one_advance_ms": round(one, 4), "per_frame_us": round(one * 1e3 / T, 2),
           "chunked_ms": {"chunk": args.chunk, "advances": len(chunks), "total": round(per, 4), "per_advance": round(per / len(chunks), 4)},
           "words_per_utterance": round(float(np.mean([len(r["words"]) for r in res])), 1),
           "reached_final": int(sum(r["reached_final"] for r in res)),
           "prefix_beam_10_one_advance_ms": round(p_one, 4), "prefix_beam_per_frame_us": round(p_one * 1e3 / T, 2),
           "data": "synthetic"}
    if args.blank_skip is not None:
        skip = CtcWfstSearch(graph, B, T, beam=args.beam, max_active=args.max_active, blank_skip=args.blank_skip)
        s_one = timed(lambda: skip.advance(logp, nf, log_softmax=False), skip.reset)
        s_res, counts = skip.result(detail=True), skip.frames()
        s_per = timed(lambda: [skip.advance(a, n, log_softmax=False) for a, n in lpc], skip.reset)
        assert [r["words"] for r in skip.result(detail=True)] == [r["words"] for r in s_res], "skipped: chunked != one-shot"
        assert skip.frames() == counts
        kept_buf, n_kept = torch.empty(B, T + 1, V, dtype=torch.float32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        sel = timed(lambda: ops.wfst_skip_select(skip.skip, skip.skip_state, logp, nf, kept_buf, n_kept),
                    lambda: ops.wfst_skip_reset(skip.skip, skip.skip_state))
        seen, kept = sum(c[0] for c in counts), sum(c[1] for c in counts)
        share = kept / max(seen, 1)
        out["blank_skip"] = {"p": args.blank_skip, "frames_seen": seen, "frames_decoded": kept, "kept_share": round(share, 4),
                             "one_advance_ms": round(s_one, 4), "per_frame_us": round(s_one * 1e3 / T, 2),
                             "select_ms": round(sel, 4), "unskipped_one_advance_ms": round(one, 4),
                             "predicted_ms": round(share * one + sel, 4),
                             "chunked_ms": {"chunk": args.chunk, "total": round(s_per, 4), "per_advance": round(s_per / len(chunks), 4)},
                             "same_words_as_unskipped": int(sum(a["words"] == b["words"] for a, b in zip(s_res, res))),
                             "reached_final": int(sum(r["reached_final"] for r in s_res))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
