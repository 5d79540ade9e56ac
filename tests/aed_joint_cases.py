"""The test cases of joint CTC/attention decoding (tests/test_aed_joint_gpu.py): models, memories, CTC log-probabilities, the
float64 reference search (tests/aed_joint_ref.py) and the float32 yardstick of each, computed once per process.

Models and memories are drawn as tests/aed_search_cases.py draws them (output_layer.bias[eos] raised so that searches end).  The
CTC log-probabilities are the float32 log-softmax of seeded random logits, made here on the CPU and given to the device as they
are, so that reference and device read the same numbers.  Weights are exactly representable in float32 (the C ABI takes a float).
The seeds were picked on the CPU so that every utterance's float64 decision margin exceeds twice the yardstick's bound and so
that the cases show what they exist for; the tests assert both, they never skip."""
import functools

import torch

import aed_joint_ref
from m3asr.config import DecoderConfig
from m3asr.weights import make_decoder_weights

REAL = dict(vocab=1434, dim=512, linear_units=2048, num_blocks=1)

SPECS = {
    # 2 blocks, D 32, dk 16, V 11, beam 3, P 5; memories of 5, 9 and 1 frames: unequal limits, m = 1 (the recursion's empty range)
    "tiny": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=3, eos_bias=0.6, mem=(5, 9, 1), beam=3, pre_beam=5, w=0.5, max_steps=None,
                 ctc_scale=2.0),
    # w = 1: attention only proposes (P = V = 5), the CTC score alone ranks
    "w1_p_is_vocab": dict(dcfg=DecoderConfig.tiny(vocab=5), seed=2, eos_bias=0.5, mem=(6, 3), beam=2, pre_beam=5, w=1.0, max_steps=None,
                          ctc_scale=2.0),
    "beam1": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=0, eos_bias=0.5, mem=(7, 4), beam=1, pre_beam=2, w=0.25, max_steps=None,
                  ctc_scale=2.0),
    "p_is_beam": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=1, eos_bias=0.5, mem=(7, 4), beam=3, pre_beam=3, w=0.5, max_steps=None,
                      ctc_scale=2.0),
    "p64": dict(dcfg=DecoderConfig.tiny(vocab=70), seed=3, eos_bias=1.0, mem=(8, 5), beam=3, pre_beam=64, w=0.5, max_steps=None,
                ctc_scale=2.0),
    # memories around the 64-frame tile of the parent's state and the 16-frame tile of the gather, and one of three tiles
    "frames": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=3, eos_bias=0.3, mem=(63, 64, 65, 130), beam=3, pre_beam=5, w=0.5, max_steps=6,
                   ctc_scale=1.0),
    "real": dict(dcfg=DecoderConfig(heads=4, **REAL), seed=1, eos_bias=1.5, mem=(70, 37), beam=4, pre_beam=6, w=0.5, max_steps=12,
                 ctc_scale=1.0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(dcfg, state dict, memory (B, T, D), mem_len, ctc log-probabilities (B, T, V) float32, spec); the draws depend on the spec only"""
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
    return dcfg, sd, memory, mem_len, ctc.float(), spec


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 search results, e32, bound) of a case: computed once, shared, never modified"""
    dcfg, sd, memory, mem_len, ctc, spec = case(name)
    r64 = aed_joint_ref.search(sd, dcfg, memory, mem_len, ctc, spec["beam"], spec["pre_beam"], spec["w"], spec["max_steps"],
                               dtype=torch.float64)
    p32 = aed_joint_ref.recomputed_parts(sd, dcfg, memory, mem_len, ctc, r64, spec["w"], dtype=torch.float32)
    e32 = aed_joint_ref.e32_of(r64, p32)
    return r64, e32, max(8 * e32, 1e-5)


# ---- what the float64 reference of an utterance shows (asserted by the tests, so that a change of seed cannot lose it)
def hits_limit_unfinished(res):
    return res["steps"] == res["limit"] and not all(h[4] for h in res["nbest"])


def repeat_steps(res, eos):
    """steps (1-based) with a kept, finitely scored candidate whose token repeats its parent's last token: the c == last branch"""
    return [i + 1 for i, e in enumerate(res["history"])
            if any(len(t) >= 2 and t[-1] == t[-2] != eos and k > -float("inf") for t, k in zip(e["tokens"], e["key"].tolist()))]


def minus_inf_steps(res):
    """steps (1-based) that keep a candidate with a -inf key"""
    return [i + 1 for i, e in enumerate(res["history"]) if any(k == -float("inf") for k in e["key"].tolist())]


def ancestry_steps(res):
    """steps (1-based, past the first) whose kept candidates share a parent while another parent has none"""
    beam = len(res["nbest"])
    return [i + 1 for i, e in enumerate(res["history"])
            if i > 0 and len(set(e["parent"])) < beam and set(e["parent"]) != set(range(beam))]
