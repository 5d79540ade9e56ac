"""Reference for the n-gram LM fusion tests (a helper, not a test): the contract restated in plain Python, independently of
m3asr/lm.py's automaton and of the library.

arpa_logp / arpa_score   the textbook ARPA scorer straight from the dict of n-grams: longest match, else back off
                         (log P(w | h) = bow(h) + log P(w | h[1:]), bow = 0 for an h that is no n-gram); no states, no tables
fused_beam_search        a pure-Python prefix beam search (the structure of oracle.ctc_decode.prefix_beam_search_topk) with the
                         rank key (log_add(pb, pnb) + bonus) + (alpha lm + beta |prefix|)
random_arpa              random valid ARPA texts whose n-gram sets are closed under the prefix rule

N-gram dicts here: {tuple of words: (log10 prob, log10 back-off weight)}; a word is a token id (int) or "<s>", "</s>", "<unk>".
"""
import math

import numpy as np

from oracle import ctc_decode as ref

LN10 = math.log(10.0)
UNK_DEFAULT = math.log(1e-10)


# ------------------------------------------------------------------------------------------------ (a) textbook scorer
def arpa_logp(grams, order, history, w, unk_default=UNK_DEFAULT):
    """natural-log P(w | history): history is the full list of words so far (with "<s>" in front if the LM has it)."""
    if (w,) not in grams:
        w = "<unk>"
    h = tuple(history[max(len(history) - (order - 1), 0):]) if order > 1 else ()

    def cond(h):
        if h + (w,) in grams:
            return grams[h + (w,)][0] * LN10
        if not h:
            return unk_default                                    # an unknown word in an LM without <unk>
        bow = grams[h][1] * LN10 if h in grams else 0.0
        return bow + cond(h[1:])

    return cond(h)


def arpa_score(grams, prefix, eos=False, unk_default=UNK_DEFAULT):
    """natural-log P(prefix) from the start of a sentence (+ log P(</s> | prefix) with eos, if the LM has </s>)."""
    order = max(len(g) for g in grams)
    hist = ["<s>"] if ("<s>",) in grams else []
    total = 0.0
    for t in prefix:
        total += arpa_logp(grams, order, hist, int(t), unk_default)
        hist.append(int(t) if (int(t),) in grams else "<unk>")
    if eos and ("</s>",) in grams:
        total += arpa_logp(grams, order, hist, "</s>", unk_default)
    return total


# ------------------------------------------------------------------------------------------------ (b) fused beam search
def fused_beam_search(top_logp, top_idx, beam, blank, graph=None, lm_walk=None, lm_final=None, alpha=0.0, beta=0.0,
                      use_eos=False):
    """graph: an object with walk(prefix) -> (state, bonus, final) or None; lm_walk(prefix) -> (lm_state, lm) or None;
    lm_final(lm_state) -> log P(</s> | state).  -> [(prefix, ctc, context final, lm (+ final with use_eos), context state)]
    ordered by (ctc + final) + (alpha lm + beta |prefix|), stable on the beam order."""
    NEG = ref.NEG_INF
    ctx_memo, lm_memo = {}, {}

    def ctx(prefix):
        if prefix not in ctx_memo:
            ctx_memo[prefix] = graph.walk(prefix) if graph is not None else (0, 0.0, 0.0)
        return ctx_memo[prefix]

    def lm(prefix):
        if prefix not in lm_memo:
            lm_memo[prefix] = lm_walk(prefix)
        return lm_memo[prefix]

    def rank_key(prefix, v):
        key = ref.log_add(*v) + ctx(prefix)[1]
        if lm_walk is not None:
            key = key + (alpha * lm(prefix)[1] + beta * len(prefix))
        return key

    beams = {(): (0.0, NEG)}
    for lp_t, ix_t in zip(np.asarray(top_logp), np.asarray(top_idx)):
        grown = {}
        for ps, s in zip((float(v) for v in lp_t), (int(v) for v in ix_t)):
            for prefix, (pb, pnb) in beams.items():
                if s == blank:
                    n_pb, n_pnb = grown.get(prefix, (NEG, NEG))
                    grown[prefix] = (ref.log_add(n_pb, pb + ps, pnb + ps), n_pnb)
                elif prefix and s == prefix[-1]:
                    n_pb, n_pnb = grown.get(prefix, (NEG, NEG))
                    grown[prefix] = (n_pb, ref.log_add(n_pnb, pnb + ps))
                    ext = prefix + (s,)
                    n_pb, n_pnb = grown.get(ext, (NEG, NEG))
                    grown[ext] = (n_pb, ref.log_add(n_pnb, pb + ps))
                else:
                    ext = prefix + (s,)
                    n_pb, n_pnb = grown.get(ext, (NEG, NEG))
                    grown[ext] = (n_pb, ref.log_add(n_pnb, pb + ps, pnb + ps))
        ranked = sorted(grown.items(), key=lambda kv: rank_key(*kv), reverse=True)
        beams = dict(ranked[:beam])
    out = []
    for p, v in beams.items():
        lmf = 0.0
        if lm_walk is not None:
            st, lmf = lm(p)
            if use_eos:
                lmf = lmf + lm_final(st)
        out.append((p, ref.log_add(*v), ctx(p)[2], lmf, ctx(p)[0]))

    def final_key(h):
        key = h[1] + h[2]
        if lm_walk is not None:
            key = key + (alpha * h[3] + beta * len(h[0]))
        return key

    return sorted(out, key=final_key, reverse=True)


# ------------------------------------------------------------------------------------------------ (c) random ARPA texts
def random_arpa(rng, V, order, n_unigrams, n_higher, bos=True, eos=True, unk=True, blank=0):
    """-> (grams, text).  Unigrams over a random choice of n_unigrams tokens (never the blank); level n takes contexts from
    level n - 1 and extends them, about n_higher n-grams per level, so every prefix of an n-gram is an n-gram.  "<s>" stands
    only first, "</s>" only last, "<unk>" only alone.  Values are rounded to four decimals, so the text holds them exactly."""
    val = lambda lo, hi: round(float(rng.uniform(lo, hi)), 4)
    toks = [t for t in range(V) if t != blank]
    words = [int(t) for t in rng.choice(toks, size=min(n_unigrams, len(toks)), replace=False)]
    levels = [{}]
    for w in words:
        levels[0][(w,)] = val(-3.0, -0.3)
    if bos:
        levels[0][("<s>",)] = -99.0
    if eos:
        levels[0][("</s>",)] = val(-2.0, -0.5)
    if unk:
        levels[0][("<unk>",)] = val(-4.0, -2.0)
    for n in range(2, order + 1):
        ctxs = [g for g in levels[-1] if g[-1] != "</s>" and g != ("<unk>",)]
        level = {}
        if ctxs:
            for _ in range(n_higher):
                c = ctxs[int(rng.integers(0, len(ctxs)))]
                w = "</s>" if eos and rng.random() < 0.1 else words[int(rng.integers(0, len(words)))]
                level[c + (w,)] = val(-2.5, -0.1)
        levels.append(level)
    extended = {g[:-1] for level in levels[1:] for g in level}
    grams = {}
    for level in levels:
        for g, lp in level.items():
            grams[g] = (lp, val(-1.0, -0.05) if g in extended else 0.0)
    return grams, arpa_text(grams)


def arpa_around(path, V, order, rng, n_unigrams=40, n_higher=150, blank=0):
    """A random LM whose unigrams cover the tokens of `path`, plus n-grams cut from the path (so that walks find arcs at
    every order) and random ones (so that they also back off)."""
    grams, _ = random_arpa(rng, V, order, n_unigrams, n_higher, blank=blank)
    val = lambda lo, hi: round(float(rng.uniform(lo, hi)), 4)
    for t in set(path):
        grams.setdefault((t,), (val(-3.0, -0.3), 0.0))
    for n in range(2, order + 1):
        for i in range(0, len(path) - n + 1, 2):
            g = tuple(path[i:i + n])
            for m in range(2, n + 1):
                grams.setdefault(g[:m], (val(-1.5, -0.05), 0.0))
    extended = {g[:-1] for g in grams if len(g) > 1}
    grams = {g: (lp, (bow if bow != 0.0 else val(-1.0, -0.05)) if g in extended else 0.0) for g, (lp, bow) in grams.items()}
    return grams, arpa_text(grams)


def arpa_text(grams):
    order = max(len(g) for g in grams)
    lines = ["", "\\data\\"]
    for n in range(1, order + 1):
        lines.append("ngram %d=%d" % (n, sum(1 for g in grams if len(g) == n)))
    for n in range(1, order + 1):
        lines += ["", "\\%d-grams:" % n]
        for g, (lp, bow) in grams.items():
            if len(g) == n:
                lines.append("%r\t%s%s" % (lp, " ".join(str(w) for w in g), "\t%r" % bow if bow != 0.0 else ""))
    lines += ["", "\\end\\", ""]
    return "\n".join(lines)
