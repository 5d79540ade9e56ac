"""The test cases of attention decoding with hotword biasing (tests/test_aed_ctx_gpu.py, tests/test_aed_ctx_host.py): models,
memories, CTC log-probabilities and LMs drawn exactly as tests/aed_lm_cases.py draws them (DecoderConfig.tiny, 2 blocks, D 32),
one or more context graphs per case, the float64 reference search (tests/aed_ctx_ref.py) and the float32 yardstick of each,
computed once per process.

The graphs are small phrase lists over the ids 1 .. V - 2 (no blank, no eos): random phrases of 2 to 4 tokens from a seeded
generator, or lists written out where a case needs a shape (a phrase that is a prefix of another, a one-token phrase, phrases
that overlap so that failure links are taken).  All phrase scores and all weights are exactly representable in float32.  The
seeds were picked on the CPU so that every utterance's float64 decision margin exceeds twice the yardstick's bound and so that
the cases show what they exist for; the tests assert both, they never skip."""
import functools

import numpy as np
import torch

import aed_ctx_ref
import aed_lm_cases
from m3asr.config import DecoderConfig
from m3asr.context import ContextGraph
from m3asr.lm import NgramLm
from m3asr.weights import make_decoder_weights

REAL = aed_lm_cases.REAL
# lm: None = no LM; graphs: a list of graph specs, dict(n, seed, score) for random phrases or dict(phrases, score); ids: graph_ids
TINY = dict(aed_lm_cases.TINY, beta=4.0, graphs=(dict(n=6, seed=1, score=2.0),), ids=None)


def _spec(**kw):
    return dict(TINY, **kw)


SPECS = {
    # the four forms on the tiny shape: V 11, beam 3, P 5, memories of 5, 9 and 1 frames
    "tiny": _spec(),                                   # CTC with LM: <true, true, true>
    "ctc": _spec(lm=None),                             # CTC alone: <true, false, true>
    "lm": _spec(w=0.0),                                # LM alone: <false, true, true>
    "att": _spec(w=0.0, lm=None),                      # neither: <false, false, true>
    "beam1": _spec(seed=0, eos_bias=0.5, mem=(7, 4), beam=1, pre_beam=2, w=0.25, beta=0.25,
                   graphs=(dict(phrases=((1,), (1, 2), (3, 4)), score=1.5),)),
    "w1_p_is_vocab": _spec(dcfg=DecoderConfig.tiny(vocab=5), seed=2, eos_bias=0.5, mem=(6, 3), beam=2, pre_beam=5, w=1.0, beta=0.25,
                           lm=dict(order=3, unigrams=3, higher=8, seed=1), graphs=(dict(phrases=((1, 2), (3,), (2, 3, 1)), score=1.5),)),
    # P = 64 of V = 70: every lane gathers
    "p64": _spec(dcfg=DecoderConfig.tiny(vocab=70), seed=3, eos_bias=1.0, mem=(8, 5), pre_beam=64, beta=0.25,
                 lm=dict(order=3, unigrams=40, higher=150, seed=1), graphs=(dict(n=40, seed=2, score=2.0),)),
    # memories around the 64-frame tile of the parent's state, the arc in front of the frame chain
    "frames": _spec(eos_bias=0.3, mem=(63, 64, 65), max_steps=6, ctc_scale=1.0, beta=0.25),
    # graph ids drawn from two graphs, -1 and G (out of range): utterances 1 and 3 are unbiased
    "mixed": _spec(mem=(5, 9, 1, 7), graphs=(dict(n=6, seed=1, score=2.0), dict(n=5, seed=2, score=3.0)), ids=(1, -1, 0, 2)),
    # failure links (overlapping phrases), a phrase that is a prefix of another, a one-token phrase
    "graphs": _spec(lm=None, graphs=(dict(phrases=((1, 2, 3), (2, 3, 4), (3,), (5, 6), (5, 6, 7, 8), (9, 1)), score=1.5),)),
    "real": _spec(dcfg=DecoderConfig(heads=4, **REAL), seed=1, eos_bias=1.5, mem=(70, 37), beam=4, pre_beam=6, max_steps=12, ctc_scale=1.0,
                  beta=0.25, lm=dict(order=3, unigrams=600, higher=1500, seed=1), graphs=(dict(n=50, seed=1, score=2.0),)),
}


def random_phrases(V, n, seed, lo=2, hi=4):
    """n distinct phrases of lo .. hi ids from 1 .. V - 2"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = tuple(int(t) for t in rng.integers(1, V - 1, size=int(rng.integers(lo, hi + 1))))
        if p not in out:
            out.append(p)
    return out


def make_graph(V, g):
    phrases = g["phrases"] if "phrases" in g else random_phrases(V, g["n"], g["seed"])
    return ContextGraph([list(p) for p in phrases], V, score=g["score"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(dcfg, state dict, memory (B, T, D), mem_len, ctc log-probabilities (B, T, V) float32, spec, NgramLm or None, [ContextGraph])"""
    spec = SPECS[name]
    dcfg = spec["dcfg"]
    g = torch.Generator().manual_seed(spec["seed"])
    sd = make_decoder_weights(dcfg, seed=spec["seed"])
    sd["after_norm.weight"] = torch.rand(dcfg.dim, generator=g) + 0.5       # the encoder's, for pack_decoder
    sd["after_norm.bias"] = torch.randn(dcfg.dim, generator=g) * 0.1
    sd["decoder.output_layer.bias"] = sd["decoder.output_layer.bias"].clone()
    sd["decoder.output_layer.bias"][dcfg.vocab - 1] += spec["eos_bias"]
    mem_len = list(spec["mem"])
    memory = torch.randn(len(mem_len), max(mem_len), dcfg.dim, generator=g)  # frames past mem_len: live numbers, to be masked
    ctc = torch.log_softmax(torch.randn(len(mem_len), max(mem_len), dcfg.vocab, generator=g) * spec["ctc_scale"], dim=-1)
    lm = NgramLm(aed_lm_cases.lm_grams(dcfg.vocab, **spec["lm"])[1], dcfg.vocab) if spec["lm"] is not None else None
    return dcfg, sd, memory, mem_len, ctc.float(), spec, lm, [make_graph(dcfg.vocab, gs) for gs in spec["graphs"]]


def _search(name, graphs, ids, dtype=torch.float64):
    dcfg, sd, memory, mem_len, ctc, spec, lm, _ = case(name)
    x = ctc if spec["w"] > 0 else None
    return aed_ctx_ref.search(sd, dcfg, memory, mem_len, x, spec["beam"], spec["pre_beam"], spec["w"], lm, spec["alpha"], spec["beta"],
                              graphs, ids, spec["use_eos"], spec["lm_on"], spec["max_steps"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 search results, e32, bound) of a case: computed once, shared, never modified"""
    dcfg, sd, memory, mem_len, ctc, spec, lm, graphs = case(name)
    x = ctc if spec["w"] > 0 else None
    r64 = _search(name, graphs, spec["ids"])
    p32 = aed_ctx_ref.recomputed_parts(sd, dcfg, memory, mem_len, x, r64, spec["w"], lm, spec["alpha"], spec["beta"], graphs, spec["ids"],
                                       spec["lm_on"], dtype=torch.float32)
    e32 = aed_ctx_ref.e32_of(r64, p32)
    return r64, e32, max(8 * e32, 1e-5)


@functools.lru_cache(maxsize=None)
def unbiased(name):
    """the float64 search of the same case with every utterance unbiased"""
    return _search(name, case(name)[7], [-1] * len(case(name)[3]))


# ---- what the float64 reference of an utterance shows (asserted by the tests, so that a change of seed cannot lose it)
def kept_bonus(res):
    """the bonus of every kept candidate of every step"""
    return [b for e in res["history"] for b in e["bonus"]]


def retractions(res):
    """(by a failed match, by eos): kept candidates whose bonus fell below their parent's at a token / at eos"""
    fail = ended = 0
    prev = None
    for e in res["history"]:
        for j, p in enumerate(e["parent"]):
            before = prev["bonus"][p] if prev is not None else 0.0
            was_finished = prev["finished"][p] if prev is not None else False
            if e["bonus"][j] < before and not was_finished:
                if e["finished"][j]:
                    ended += 1
                else:
                    fail += 1
        prev = e
    return fail, ended


def ancestry_steps(res):
    return aed_lm_cases.ancestry_steps(res)
