#!/usr/bin/env python3
"""Attention decoding timed: 16 utterances x beam 10 at real dimensions (D 512, 4 heads, F 2048, V 1434,
6 blocks; 125 memory frames = 5 s of audio), synthetic weights.  With random weights eos has probability about 1 / V and every
search would run to its limit, so output_layer.bias[eos] is raised by --eos-bias.  The JSON line reports what the searches did
(steps taken, hypothesis lengths); see DESIGN.md 21 for what the default gives and why no bias gives a uniform beam.  The
memory lengths are drawn from [frames / 2, frames] as tools/bench_rescore.py draws them (the JSON line says which);
--full-length gives every utterance all --frames frames.

  python tools/bench_attention_search.py [--batch 16] [--beam 10] [--frames 125] [--blocks 6] [--rounds 10] [--graph]
                                         [--ctc-weight W [--pre-beam K]] [--lm N_NGRAMS | --lm-image FILE.npy] [--lm-weight A] [--length-bonus B] [--table]

--ctc-weight W > 0 times the joint CTC/attention search on the same model and memories.  Its CTC output is
synthetic too, but shaped like a trained model's: every utterance has a hidden token sequence of mem_len // 6 tokens, one spike
every sixth frame and blank in between (logit +10 on the frame's target over unit noise), so the CTC part has an opinion on
how long a hypothesis should be; the JSON line reports those lengths next to the hypotheses'.  The eager restatement is the
attention-only search and is skipped in this mode.

--lm N times the search with a synthetic trigram LM of about N n-grams (tools/lm_synth.py, as tools/bench_ctc_beam.py --lm
draws it; or --lm-image: an image saved by m3asr.lm.NgramLm.save, the compile of a large LM takes minutes) fused in NEXT TO the unfused search of the same build, model, memories and --ctc-weight ("fused_*"
beside "device_*"), and reports the fused hypotheses' lengths.  --table also prints one JSON line per (lm_weight, length_bonus)
in {0, --lm-weight} x {0, 1, 2, 4, 6} with the lengths (all hypotheses and the best of each beam) and the finished count: one search
each, nothing timed.  The weights are synthetic: the table shows lengths, not accuracy.

--context N times the search biased by a context graph of N random phrases of 2 to 4 tokens (--context-score per
token) NEXT TO the plain search of the same build, model, memories and --ctc-weight ("biased_*" beside "device_*"); with --lm
the biased search is fused with the LM too.  With --ctc-weight 0 and no LM the plain search has no pre-beam (8 L + 3 launches),
the biased one has (8 L + 4).

"device": wall time of AttentionBeamSearch.search() per call -- the K / V GEMM, every step's launches, the polls of the done
flags and the read of the results -- median over the rounds after a warm-up; us per step = that over the steps issued.
"eager": the same search as tests/aed_search_ref.py states it -- every hypothesis on its own, the prefix recomputed at every
step, plain torch float32 -- on the same GPU, timed --eager-rounds times (default 1; 0 skips it) after a warm-up search
of the first utterance for two steps, which loads every kernel the eager path uses.  --graph also times the captured step
and checks that it leaves the same bits.  Prints one JSON line; the results are compared before anything is timed."""
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

from m3asr.config import DecoderConfig
from m3asr.weights import make_decoder_weights


def make_case(batch, frames, blocks, eos_bias, seed=0, full_length=False):
    dcfg = DecoderConfig(vocab=1434, dim=512, heads=4, linear_units=2048, num_blocks=blocks)
    sd = make_decoder_weights(dcfg, seed=seed)
    g = torch.Generator().manual_seed(seed)
    sd["after_norm.weight"], sd["after_norm.bias"] = torch.ones(dcfg.dim), torch.zeros(dcfg.dim)
    sd["decoder.output_layer.bias"] = sd["decoder.output_layer.bias"].clone()
    sd["decoder.output_layer.bias"][-1] += eos_bias
    memory = torch.randn(batch, frames, dcfg.dim, generator=g)
    mem_len = torch.randint(frames // 2, frames + 1, (batch,), generator=g).to(torch.int32)
    if full_length:
        mem_len = torch.full((batch,), frames, dtype=torch.int32)
    return dcfg, sd, memory, mem_len


def make_ctc(mem_len, frames, vocab, seed=1):
    """(B, frames, V) CTC logits with a hidden target per utterance, and the targets' lengths"""
    g = torch.Generator().manual_seed(seed)
    B = mem_len.numel()
    logits = torch.randn(B, frames, vocab, generator=g)
    n_tok = []
    for b in range(B):
        m = int(mem_len[b])
        target = torch.zeros(frames, dtype=torch.long)                      # blank
        pos = torch.arange(3, m, 6)
        target[pos] = torch.randint(1, vocab - 1, (pos.numel(),), generator=g)
        logits[b, torch.arange(frames), target] += 10.0
        n_tok.append(int(pos.numel()))
    return logits, n_tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--eos-bias", type=float, default=1.2)
    ap.add_argument("--max-steps", type=int, default=None, help="default: --frames")
    ap.add_argument("--poll", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--eager-rounds", type=int, default=1)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--full-length", action="store_true")
    ap.add_argument("--ctc-weight", type=float, default=0.0, help="above 0: the joint CTC/attention search with this weight")
    ap.add_argument("--pre-beam", type=int, default=None, help="--ctc-weight: candidates per hypothesis for the CTC scorer")
    ap.add_argument("--lm", type=int, default=None, metavar="N_NGRAMS", help="also time the search with a synthetic LM of N n-grams fused in")
    ap.add_argument("--lm-image", default=None, metavar="FILE.npy", help="a compiled LM image instead of --lm")
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--length-bonus", type=float, default=0.0)
    ap.add_argument("--table", action="store_true", help="--lm: the hypothesis-length table over lm_weight x length_bonus")
    ap.add_argument("--context", type=int, default=None, metavar="N_PHRASES", help="also time the search biased by N random phrases of 2 to 4 tokens")
    ap.add_argument("--context-score", type=float, default=2.0)
    a = ap.parse_args()
    import aed_search_ref
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.plan import pack_decoder
    from m3asr.rescore import AttentionRescorer
    dcfg, sd, memory, mem_len = make_case(a.batch, a.frames, a.blocks, a.eos_bias, full_length=a.full_length)
    B, beam, steps = a.batch, a.beam, a.max_steps or a.frames
    res = AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")
    joint = dict(ctc_weight=a.ctc_weight, pre_beam=a.pre_beam) if a.ctc_weight > 0 else {}
    lm = None
    if a.lm_image:
        from m3asr.lm import NgramLm
        lm = NgramLm.load(a.lm_image).to("cuda:0")
    elif a.lm is not None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from lm_synth import synthetic_lm
        lm = synthetic_lm(a.lm, dcfg.vocab).to("cuda:0")
    search = AttentionBeamSearch(res, B, beam, steps, poll=a.poll, **joint)
    mem_d = memory.cuda()
    call = {}
    if joint:
        ctc, n_tok = make_ctc(mem_len, a.frames, dcfg.vocab)
        call = dict(ctc_logits=ctc.cuda())
    out = search.search(mem_d, mem_len, detail=True, **call)
    taken = search.last["steps"].cpu().tolist()
    lengths = [len(h[0]) for u in out for h in u[1]]
    record = {"metric": "attention decoding, %d utterances x beam %d, %d blocks, D 512 / F 2048 / V 1434, %d frames" % (
        B, beam, a.blocks, a.frames), "mem_len_min_max": [int(mem_len.min()), int(mem_len.max())], "eos_bias": a.eos_bias, "steps_taken_min_max": [min(taken), max(taken)],
        "hyp_tokens_min_median_max": [min(lengths), statistics.median(lengths), max(lengths)],
        "finished": "%d/%d" % (sum(int(h[2]) for u in out for h in u[1]), B * beam),
        "launches_per_step": search.launches_per_step(), "poll": a.poll, "data": "synthetic"}
    if joint:
        best = [len(u[0]) for u in out]
        record.update(ctc_weight=a.ctc_weight, pre_beam=search.pre_beam, ctc_target_tokens_min_median_max=[min(n_tok), statistics.median(n_tok), max(n_tok)],
                      best_hyp_tokens_min_median_max=[min(best), statistics.median(best), max(best)],
                      best_minus_target_min_max=[min(x - y for x, y in zip(best, n_tok)), max(x - y for x, y in zip(best, n_tok))])

    def timed(f, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def add(tag, s, ts):
        record[tag + "_ms_median"] = round(statistics.median(ts), 3)
        record[tag + "_ms_min"] = round(min(ts), 3)
        record[tag + "_steps_issued"] = s.steps_issued
        record[tag + "_us_per_step"] = round(statistics.median(ts) * 1e3 / max(s.steps_issued, 1), 1)

    timed(lambda: search.search(mem_d, mem_len, **call), 3)
    add("device", search, timed(lambda: search.search(mem_d, mem_len, **call), a.rounds))
    if lm is not None:
        def lengths_of(o):
            every, best = [len(h[0]) for u in o for h in u[1]], [len(u[0]) for u in o]
            return dict(hyp_tokens_min_median_max=[min(every), statistics.median(every), max(every)],
                        best_hyp_tokens_min_median_max=[min(best), statistics.median(best), max(best)],
                        finished="%d/%d" % (sum(int(h[2]) for u in o for h in u[1]), B * beam))

        fused = AttentionBeamSearch(res, B, beam, steps, poll=a.poll, ctc_weight=a.ctc_weight, pre_beam=a.pre_beam, lm=lm,
                                    lm_weight=a.lm_weight, length_bonus=a.length_bonus)
        fout = fused.search(mem_d, mem_len, detail=True, **call)
        record["lm"] = dict(n_grams=lm.n_grams, order=lm.order, states=lm.n_states, arcs=lm.n_arcs, image_bytes=int(lm.image.nbytes),
                            lm_weight=a.lm_weight, length_bonus=a.length_bonus, pre_beam=fused.pre_beam,
                            launches_per_step=fused.launches_per_step(), **lengths_of(fout))
        timed(lambda: fused.search(mem_d, mem_len, **call), 3)
        add("fused", fused, timed(lambda: fused.search(mem_d, mem_len, **call), a.rounds))
        record["fused_over_device"] = round(record["fused_ms_median"] / record["device_ms_median"], 3)
        if a.table:
            for lw in sorted({0.0, a.lm_weight}):
                for lb in (0.0, 1.0, 2.0, 4.0, 6.0):
                    fused.lm_weight, fused.length_bonus = lw, lb            # run-time arguments of the score launch
                    row = lengths_of(fused.search(mem_d, mem_len, detail=True, **call))
                    print(json.dumps(dict(table="hypothesis lengths", eos_bias=a.eos_bias, ctc_weight=a.ctc_weight, max_steps=steps,
                                          lm_weight=lw, length_bonus=lb, steps_issued=fused.steps_issued, **row)))
    if a.context is not None:
        import numpy as np
        from m3asr.context import ContextGraph, ContextSet
        rng = np.random.default_rng(7)
        phrases = set()
        while len(phrases) < a.context:
            phrases.add(tuple(int(t) for t in rng.integers(1, dcfg.vocab - 1, size=int(rng.integers(2, 5)))))
        graph = ContextGraph([list(p) for p in sorted(phrases)], dcfg.vocab, score=a.context_score)
        ctx = ContextSet([graph], device="cuda:0")
        lmkw = dict(lm=lm, lm_weight=a.lm_weight, length_bonus=a.length_bonus) if lm is not None else {}
        biased = AttentionBeamSearch(res, B, beam, steps, poll=a.poll, ctc_weight=a.ctc_weight, pre_beam=a.pre_beam, context=ctx, **lmkw)
        bout = biased.search(mem_d, mem_len, detail=True, **call)
        bonus = [h[-2] for u in bout for h in u[1]]
        record["context"] = dict(phrases=len(graph.phrases), states=graph.n_states, columns=graph.A, image_bytes=int(ctx.image.nbytes),
                                 score=a.context_score, pre_beam=biased.pre_beam, launches_per_step=biased.launches_per_step(),
                                 with_lm=lm is not None, hyps_with_bonus="%d/%d" % (sum(1 for v in bonus if v != 0), len(bonus)),
                                 finished="%d/%d" % (sum(int(h[2]) for u in bout for h in u[1]), B * beam))
        timed(lambda: biased.search(mem_d, mem_len, **call), 3)
        add("biased", biased, timed(lambda: biased.search(mem_d, mem_len, **call), a.rounds))
        record["biased_over_device"] = round(record["biased_ms_median"] / record["device_ms_median"], 3)
    if a.graph:
        graphed =AttentionBeamSearch(res, B, beam, steps, poll=a.poll, use_graph=True, **joint)
        same = graphed.search(mem_d, mem_len, detail=True, **call) == out
        same = same and torch.equal(graphed.last["score"].view(torch.int32), search.last["score"].view(torch.int32))
        record["graph_same_bits"] = bool(same)
        timed(lambda: graphed.search(mem_d, mem_len, **call), 3)
        add("graph", graphed, timed(lambda: graphed.search(mem_d, mem_len, **call), a.rounds))
    if a.eager_rounds > 0 and not joint:
        sd_d = {k: v.cuda() for k, v in sd.items()}

        def eager():
            r = aed_search_ref.search(sd_d, dcfg, mem_d, mem_len.tolist(), beam, steps, dtype=torch.float32)
            torch.cuda.synchronize()
            return r

        aed_search_ref.search(sd_d, dcfg, mem_d[:1], mem_len[:1].tolist(), beam, 2, dtype=torch.float32)     # warm-up
        ref = eager()
        eag = timed(eager, a.eager_rounds)
        record["eager_aed_search_ref_ms_median"] = round(statistics.median(eag), 1)
        record["same_best_as_eager"] = "%d/%d" % (sum(int(tuple(u[0]) == r["nbest"][r["best"]][0]) for u, r in zip(out, ref)), B)
        record["max_abs_score_diff_vs_eager"] = max(abs(h[1] - w[1]) for u, r in zip(out, ref) for h, w in zip(u[1], r["nbest"])
                                                    if h[0] == w[0])
    print(json.dumps(record))


if __name__ == "__main__":
    main()
