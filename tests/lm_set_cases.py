"""The cases of the LM-set tests (a helper, not a test): three members over V = 16 and the inputs they are searched on.

Members: orders 1, 2 and 3 (tests/lm_ref.random_arpa over all 15 non-blank tokens), the bigram LM without <s>, so that start
states, state counts and tables all differ; scales (1.0, 0.5, 2.0), all exact in float32.  The oracle of every GPU test is the
code that exists without sets: an utterance that picks member j must get the BITS of the single-LM search with lms[j] and
lm_weight = ALPHA * float32(scale_j), the product formed in double.

Seeds were picked on the CPU so that the members are SELECTIVE on every utterance (tests/test_lm_set_host.py asserts it with the
host routine): under the three members hyp_lm is pairwise different and at least two best hypotheses differ, so a kernel that
walks the wrong member, takes the wrong scale or starts in another member's start state cannot pass."""
import functools

import numpy as np
import torch

import lm_ref

V, BLANK = 16, 0
ALPHA, BETA = 0.75, 0.25
SCALES = (1.0, 0.5, 2.0)
MEMBERS = (dict(order=1, bos=True, higher=0, seed=11), dict(order=2, bos=False, higher=60, seed=12),
           dict(order=3, bos=True, higher=90, seed=13))
B, T, BEAM = 4, 20, 4
LM_ON = (3, 0, 1, 2)


def weight(j, alpha=ALPHA):
    """the single-LM search's lm_weight that member j's utterances are compared with: one double product"""
    return alpha * float(np.float32(SCALES[j]))


@functools.lru_cache(maxsize=None)
def arpa_texts():
    return tuple(lm_ref.random_arpa(np.random.default_rng(m["seed"]), V, m["order"], V - 1, m["higher"], bos=m["bos"])[1]
                 for m in MEMBERS)


def members():
    """three fresh NgramLm (host side)"""
    from m3asr.lm import NgramLm
    return [NgramLm.from_arpa(t, None, blank=BLANK, vocab_size=V) for t in arpa_texts()]


def lm_set():
    from m3asr.lm import NgramLmSet
    return NgramLmSet(members(), SCALES)


@functools.lru_cache(maxsize=None)
def ctc_logits(seed=5, n=B, frames=T):
    """(n, frames, V) logits with a blank-heavy frame in every fourth position; computed once, never modified"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, frames, V, generator=g) * 2.0
    x[:, ::4, BLANK] += 2.5
    return x


def host_topk(x, k):
    """per-frame log-softmax and the k best (value desc, index asc) of x (T, V) on the CPU, float32, as numpy"""
    lp = torch.log_softmax(x.float(), dim=-1)
    order = torch.argsort(-lp, dim=-1, stable=True)[:, :k]
    return torch.gather(lp, 1, order).numpy(), order.to(torch.int32).numpy()


def host_search(x, lm_image, alpha, beam=BEAM, beta=BETA):
    """the library's host routine over the CPU top-k of x (T, V): [(prefix, ctc, bonus, lm, state)]"""
    from m3asr import ops
    lp, ix = host_topk(x, beam)
    return ops.ctc_prefix_beam_search_lm_host(lp, ix, beam, BLANK, None, -1, lm_image, alpha, beta, True)
