"""The graphs, scores and settings that the WFST tests share (CPU and GPU tier): generated here, from fixed seeds, so that the
host test can show that the cases exercise every mechanism of the contract and the device test runs exactly those cases."""
import math

import numpy as np

from m3asr.wfst import DecodingGraph

WEIGHTS = np.array([-1.0, -0.5, 0.0, 0.0, 0.25, 0.5, 0.5, 1.0, 2.0])          # dyadic: sums are exact, ties are frequent
LOGPS = np.array([-0.25, -0.5, -0.5, -1.0, -1.0, -2.0, -4.0])
BEAMS = (0.5, 4.0, math.inf)
MAX_ACTIVE = (1, 2, 5, None)                                                    # None = n_states


def random_graph(rng, n_states, V, depth, arcs_per_state=3.0, p_eps=0.35, p_out=0.4, n_words=5, p_final=0.4, p_no_emit=0.1):
    """A random transducer whose epsilon-input subgraph is acyclic: every state gets a rank in [0, depth] and an epsilon arc
    only climbs in rank."""
    rank = rng.integers(0, depth + 1, n_states)
    rank[:min(depth + 1, n_states)] = np.arange(min(depth + 1, n_states))         # one chain of epsilon arcs through every rank
    src, dst, il, ol, w = [], [], [], [], []
    for s in range(min(depth, n_states - 1)):
        src.append(s), dst.append(s + 1), il.append(0), ol.append(int(rng.integers(0, n_words + 1))), w.append(float(rng.choice(WEIGHTS)))
    for s in range(n_states):
        if s == 0 or rng.random() >= p_no_emit:
            for _ in range(max(1, rng.poisson(arcs_per_state))):
                src.append(s), dst.append(int(rng.integers(n_states))), il.append(int(rng.integers(1, V + 1)))
                ol.append(int(rng.integers(1, n_words + 1)) if rng.random() < p_out else 0), w.append(float(rng.choice(WEIGHTS)))
        higher = np.flatnonzero(rank > rank[s])
        if higher.size and rng.random() < p_eps:
            for d in rng.choice(higher, size=min(higher.size, int(rng.integers(1, 3))), replace=False):
                src.append(s), dst.append(int(d)), il.append(0)
                ol.append(int(rng.integers(1, n_words + 1)) if rng.random() < p_out else 0), w.append(float(rng.choice(WEIGHTS)))
    fin = np.where(rng.random(n_states) < p_final, rng.choice(np.abs(WEIGHTS), n_states), np.inf)
    fin[int(rng.integers(n_states))] = 0.0
    return DecodingGraph(n_states, 0, src, dst, il, ol, w, fin, V)


def random_logp(rng, T, V, p_inf=0.02):
    x = rng.choice(LOGPS, size=(T, V)).astype(np.float32)
    x[rng.random((T, V)) < p_inf] = -np.inf
    return x


def random_case(seed):
    """dict(graph, logp (T, V), beam, max_active, seed): sizes and settings from the seed."""
    rng = np.random.default_rng(1000 + seed)
    n_states, V, T = int(rng.integers(6, 41)), int(rng.integers(3, 7)), int(rng.integers(1, 61))
    depth = int(rng.integers(0, 6))
    g = random_graph(rng, n_states, V, depth)
    ma = MAX_ACTIVE[(seed // 3) % 4]
    return dict(seed=seed, graph=g, logp=random_logp(rng, T, V), beam=BEAMS[seed % 3], max_active=n_states if ma is None else ma)


RANDOM_SEEDS = tuple(range(36))                                                 # every (beam, max_active) pair three times


def tiny_case(seed):
    """A graph of at most 12 states for the exhaustive trellis."""
    rng = np.random.default_rng(5000 + seed)
    n_states, V, T = int(rng.integers(2, 13)), int(rng.integers(2, 5)), int(rng.integers(0, 9))
    g = random_graph(rng, n_states, V, int(rng.integers(0, 4)), arcs_per_state=2.5, p_eps=0.5)
    return dict(seed=seed, graph=g, logp=random_logp(rng, T, V))


def wide_graph(n_fan, V=4):
    """Start state 0 with an emitting arc to each of n_fan leaf states (ilabels cycling, weights dyadic by leaf), every leaf
    looping on every label and final: after the first frame exactly n_fan + 1 states are live (the start keeps a self-loop).
    Leaves carry a word on the way in; ties between leaves are frequent."""
    src, dst, il, ol, w = [0], [0], [1], [0], [0.0]
    for i in range(n_fan):
        leaf = 1 + i
        src.append(0), dst.append(leaf), il.append(1 + i % V), ol.append(1 + i % 7), w.append(0.25 * (i % 5))
        for v in range(V):
            src.append(leaf), dst.append(leaf), il.append(v + 1), ol.append(0), w.append(0.5 * (v % 2))
    fin = np.zeros(n_fan + 1)
    fin[0] = np.inf
    return DecodingGraph(n_fan + 1, 0, src, dst, il, ol, w, fin, V)


def flat_logp(T, V, seed=0):
    rng = np.random.default_rng(seed)
    return rng.choice(LOGPS, size=(T, V)).astype(np.float32)


TOY_LEXICON = {1: [1, 2], 2: [1, 2, 3], 3: [3, 3], 4: [2, 1]}                  # 1 / 2 share a prefix; 3 doubles a token; 2 ends in what 3 starts with


def peaked_logits(alignment, V, peak=8.0):
    """(T, V) logits with `peak` on the alignment's token of each frame, 0 elsewhere."""
    x = np.zeros((len(alignment), V), dtype=np.float32)
    x[np.arange(len(alignment)), alignment] = peak
    return x
