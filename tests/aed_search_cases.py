"""The test cases of attention decoding, shared by tests/test_aed_search_host.py (CPU) and tests/test_aed_search_gpu.py: models,
memories, the float64 reference search and the float32 yardstick of each, computed once per process.

Test models must end: with random weights eos has probability about 1 / V and every search would run to its limit, so every
case raises output_layer.bias[eos] in its state dict (`eos_bias` below; the host test checks on the CPU what the value does).
The seeds and biases were picked on the CPU so that the cases together show finished and live slots side by side, a stop before
the limit, a stop at the limit with unfinished slots, and a pruning step that needs the ancestry table -- and so that every
utterance's float64 decision margin exceeds twice the yardstick's bound.  The tests assert all of that; they never skip."""
import functools

import torch

import aed_search_ref
from m3asr.config import DecoderConfig
from m3asr.weights import make_decoder_weights

REAL = dict(vocab=1434, dim=512, linear_units=2048, num_blocks=1)

SPECS = {
    # 2 blocks, D 32, 2 heads (dk 16), F 64, V 11; unequal limits, early freezing, limit = 1
    "tiny": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=17, eos_bias=0.6, mem=(5, 9, 1), beam=3, max_steps=None),
    "tiny_cap4": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=17, eos_bias=0.6, mem=(5, 9, 1), beam=3, max_steps=4),
    "beam1": dict(dcfg=DecoderConfig.tiny(vocab=11), seed=5, eos_bias=0.5, mem=(7, 4), beam=1, max_steps=None),
    "beam_is_vocab": dict(dcfg=DecoderConfig.tiny(vocab=5), seed=5, eos_bias=0.5, mem=(6, 3), beam=5, max_steps=None),
    "real_h4": dict(dcfg=DecoderConfig(heads=4, **REAL), seed=13, eos_bias=1.5, mem=(70, 37), beam=4, max_steps=12),
    "real_h8": dict(dcfg=DecoderConfig(heads=8, **REAL), seed=14, eos_bias=1.0, mem=(70, 37), beam=4, max_steps=12),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(dcfg, state dict, memory (B, T, D), mem_len, beam, max_steps); the random draws depend on the spec only"""
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
    return dcfg, sd, memory, mem_len, spec["beam"], spec["max_steps"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 search results, e32, bound) of a case: computed once, shared, never modified"""
    dcfg, sd, memory, mem_len, beam, max_steps = case(name)
    r64 = aed_search_ref.search(sd, dcfg, memory, mem_len, beam, max_steps, dtype=torch.float64)
    s32 = aed_search_ref.teacher_forced_scores(sd, dcfg, memory, mem_len, r64, dtype=torch.float32)
    e32 = aed_search_ref.e32_of(r64, s32)
    return r64, e32, max(8 * e32, 1e-5)


# ---- what the float64 reference of an utterance shows (asserted by the tests, so that a change of seed cannot lose it)
def coexist_steps(res):
    """steps after which finished and live slots stand side by side"""
    return sum(1 for e in res["history"] if any(e["finished"]) and not all(e["finished"]))


def stops_early(res):
    return res["steps"] < res["limit"] and all(f for _, _, f in res["nbest"])


def hits_limit_unfinished(res):
    return res["steps"] == res["limit"] and not all(f for _, _, f in res["nbest"])


def ancestry_steps(res):
    """steps (1-based, past the first) whose kept candidates share a parent while another parent has none"""
    beam = len(res["nbest"])
    return [i + 1 for i, e in enumerate(res["history"])
            if i > 0 and len(set(e["parent"])) < beam and set(e["parent"]) != set(range(beam))]
