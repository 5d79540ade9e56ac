"""A synthetic n-gram LM of N n-grams above the unigrams for the decode benchmarks (tools/bench_ctc_beam.py, tools/bench_streaming.py):
unigrams over every token but the blank, <s> and </s>, the rest as bigrams (1/3) and trigrams (2/3) whose contexts are drawn
from the level below, so the set is closed under the prefix rule.  Values are random: the benchmarks time the walk, and the
walk's cost depends on the shape of the automaton (states, arcs per state, back-off depth), not on the probabilities."""
import math

import numpy as np

from m3asr.lm import BOS, EOS, NgramLm


def synthetic_lm(n_grams, vocab_size, seed=0, blank=0):
    rng = np.random.default_rng(seed)
    toks = [t for t in range(vocab_size) if t != blank]
    grams = {(t,): (float(v), 0.0) for t, v in zip(toks, rng.uniform(-9.0, -2.0, len(toks)))}
    grams[(BOS,)] = (-99.0 * math.log(10.0), 0.0)
    grams[(EOS,)] = (-3.0, 0.0)
    rest = max(int(n_grams), 3)
    prev = [g for g in grams if g != (EOS,)]
    for order, want in ((2, rest // 3), (3, rest - rest // 3)):
        level, tries = {}, 0
        ctx = rng.integers(0, len(prev), 2 * want + 16)
        tok = rng.integers(0, len(toks), 2 * want + 16)
        val = rng.uniform(-6.0, -0.1, 2 * want + 16)
        while len(level) < want and tries < ctx.size:
            level[prev[ctx[tries]] + (toks[tok[tries]],)] = (float(val[tries]), 0.0)
            tries += 1
        grams.update(level)
        prev = list(level)
    extended = {g[:-1] for g in grams if len(g) > 1}
    bow = rng.uniform(-2.0, -0.05, len(extended))
    for g, b in zip(extended, bow):
        grams[g] = (grams[g][0], float(b))
    return NgramLm(grams, vocab_size, blank)
