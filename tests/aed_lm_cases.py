"""The test cases of attention decoding with LM fusion (tests/test_aed_lm_gpu.py, tests/test_aed_lm_host.py): models, memories
and CTC log-probabilities drawn as tests/aed_joint_cases.py draws them, an n-gram LM per case, the float64 reference search
(tests/aed_lm_ref.py) and the float32 yardstick of each, computed once per process.

The LMs are small random gram dicts (tests/lm_ref.random_arpa: orders 1, 2 and 3, <s>, </s> and <unk> present, contexts without the
extension asked for, so that walks back off; unigrams over a part of the vocabulary, so that some tokens are unknown) compiled with
NgramLm(grams, V).  All weights (ctc_weight, lm_weight, length_bonus) are exactly representable in float32.  The seeds were
picked on the CPU so that every utterance's float64 decision margin exceeds twice the yardstick's bound and so that the cases
show what they exist for; the tests assert both, they never skip."""
import functools

import numpy as np
import torch

import aed_lm_ref
import lm_ref
from m3asr.config import DecoderConfig
from m3asr.lm import BOS, EOS, UNK, NgramLm
from m3asr.weights import make_decoder_weights

REAL = dict(vocab=1434, dim=512, linear_units=2048, num_blocks=1)
TINY = dict(dcfg=DecoderConfig.tiny(vocab=11), seed=3, eos_bias=0.6, mem=(5, 9, 1), beam=3, pre_beam=5, w=0.5, max_steps=None,
            ctc_scale=2.0, alpha=0.5, beta=0.25, use_eos=True, lm_on=None, lm=dict(order=3, unigrams=7, higher=30, seed=1))


def _spec(**kw):
    return dict(TINY, **kw)


SPECS = {
    # 2 blocks, D 32, dk 16, V 11, beam 3, P 5; memories of 5, 9 and 1 frames; a trigram LM over 7 of the 10 non-blank ids.  A live
    # hypothesis of this model loses about 3.5 per token (the CTC columns are drawn with scale 2), so it takes a bonus of 4 per
    # token to keep hypotheses alive past the ones that ended early
    "tiny": _spec(beta=4.0),
    # the same search without the length bonus: what tiny's beta is measured against (tests/test_aed_lm_host.py)
    "tiny_beta0": _spec(beta=0.0),
    # order 1: every walk is state 0
    "unigram": _spec(lm=dict(order=1, unigrams=7, higher=0, seed=2)),
    # order 2: one level above state 0
    "bigram": _spec(lm=dict(order=2, unigrams=7, higher=20, seed=3)),
    # a kept candidate that backs off two levels, and one that lands on unk_logp
    "backoff": _spec(lm=dict(order=3, unigrams=5, higher=12, seed=4), alpha=0.25),
    # ctc_weight = 0: attention plus LM, the <false, true> instantiation
    "w0": _spec(w=0.0),
    "w1_p_is_vocab": _spec(dcfg=DecoderConfig.tiny(vocab=5), seed=2, eos_bias=0.5, mem=(6, 3), beam=2, pre_beam=5, w=1.0,
                           lm=dict(order=3, unigrams=3, higher=8, seed=1)),
    "beam1": _spec(seed=0, eos_bias=0.5, mem=(7, 4), beam=1, pre_beam=2, w=0.25),
    # P = 64 of V = 70: every lane walks
    "p64": _spec(dcfg=DecoderConfig.tiny(vocab=70), seed=3, eos_bias=1.0, mem=(8, 5), pre_beam=64, lm=dict(order=3, unigrams=40, higher=150, seed=1)),
    # memories around the 64-frame tile of the parent's state, with the walk in front of the frame chain
    "frames": _spec(eos_bias=0.3, mem=(63, 64, 65), max_steps=6, ctc_scale=1.0),
    "no_eos": _spec(use_eos=False),
    "beta_only": _spec(alpha=0.0, beta=0.5),
    "mixed": _spec(beta=4.0, lm_on=(1, 0, 1)),
    "zero_weights": _spec(alpha=0.0, beta=0.0),
    "real": _spec(dcfg=DecoderConfig(heads=4, **REAL), seed=1, eos_bias=1.5, mem=(70, 37), beam=4, pre_beam=6, max_steps=12, ctc_scale=1.0,
                  lm=dict(order=3, unigrams=600, higher=1500, seed=1)),
}
_WORDS = {"<s>": BOS, "</s>": EOS, "<unk>": UNK}


def lm_grams(V, order, unigrams, higher, seed):
    """(the log10 dict of tests/lm_ref.py, the same n-grams as NgramLm takes them: ids, natural logs)"""
    grams10, _ = lm_ref.random_arpa(np.random.default_rng(seed), V, order, unigrams, higher)
    grams = {tuple(_WORDS.get(t, t) for t in g): (lp * lm_ref.LN10, bow * lm_ref.LN10) for g, (lp, bow) in grams10.items()}
    return grams10, grams


@functools.lru_cache(maxsize=None)
def case(name):
    """(dcfg, state dict, memory (B, T, D), mem_len, ctc log-probabilities (B, T, V) float32, spec, NgramLm, its log10 dict)"""
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
    grams10, grams = lm_grams(dcfg.vocab, **spec["lm"])
    return dcfg, sd, memory, mem_len, ctc.float(), spec, NgramLm(grams, dcfg.vocab), grams10


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 search results, e32, bound) of a case: computed once, shared, never modified"""
    dcfg, sd, memory, mem_len, ctc, spec, lm, _ = case(name)
    x = ctc if spec["w"] > 0 else None
    r64 = aed_lm_ref.search(sd, dcfg, memory, mem_len, x, spec["beam"], spec["pre_beam"], spec["w"], lm, spec["alpha"], spec["beta"],
                            spec["use_eos"], spec["lm_on"], spec["max_steps"], dtype=torch.float64)
    p32 = aed_lm_ref.recomputed_parts(sd, dcfg, memory, mem_len, x, r64, spec["w"], spec["alpha"], spec["beta"], spec["lm_on"],
                                      dtype=torch.float32)
    e32 = aed_lm_ref.e32_of(r64, p32)
    return r64, e32, max(8 * e32, 1e-5)


# ---- what the float64 reference of an utterance shows (asserted by the tests, so that a change of seed cannot lose it)
def kept_levels(res):
    """the back-off levels of every kept candidate of every step"""
    return [lv for e in res["history"] for lv in e["levels"]]


def kept_unknown(res):
    """how many kept, finitely scored candidates landed on unk_logp"""
    return sum(1 for e in res["history"] for u, k in zip(e["unk"], e["key"].tolist()) if u and k > -float("inf"))


def ancestry_steps(res):
    """steps (1-based, past the first) whose kept candidates share a parent while another parent has none"""
    beam = len(res["nbest"])
    return [i + 1 for i, e in enumerate(res["history"])
            if i > 0 and len(set(e["parent"])) < beam and set(e["parent"]) != set(range(beam))]


def shortest_finished(results):
    """the token count of the shortest finished hypothesis over all utterances (None: nothing finished)"""
    lens = [len(h[0]) for r in results for h in r["nbest"] if h[4]]
    return min(lens) if lens else None
