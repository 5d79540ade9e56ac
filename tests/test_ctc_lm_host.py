"""N-gram LM shallow fusion of the CTC prefix beam search, host side: the ARPA compiler (m3asr.lm.NgramLm), the image check
(m3_ctc_lm_validate) and the fused host search (m3_ctc_prefix_beam_search_lm), which is the yardstick of the device search
(tests/test_ctc_lm_gpu.py).

Yardsticks here (tests/lm_ref.py): a textbook ARPA scorer that knows nothing of states or tables; a pure-Python prefix beam
search with the fused rank key on the same top-k pairs -- prefixes and order identical, ctc, bonus and lm to 1e-6, the bound
tests/test_ctc_beam_gpu.py uses between device and host; random ARPA texts; and a normalised LM (absolute discounting over a
toy corpus) whose automaton must sum to one in every reachable state.
"""
import ctypes
import math
import os
import re
from collections import Counter

import numpy as np
import pytest

import lm_ref
from oracle import ctc_decode as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lm(text, V, **kw):
    from m3asr.lm import NgramLm
    return NgramLm.from_arpa(text, None, blank=0, vocab_size=V, **kw)


def _variants():
    """(order, bos, eos, unk): orders 1..4, with and without the three special words"""
    out = []
    for order in (1, 2, 3, 4):
        for flags in ((True, True, True), (False, False, False), (True, True, False), (False, True, True)):
            out.append((order,) + flags)
    return out


# ------------------------------------------------------------------------------------------------ 1. score == textbook
@pytest.mark.parametrize("order,bos,eos,unk", _variants())
def test_score_is_the_textbook_arpa_score(order, bos, eos, unk):
    V = 12
    rng = np.random.default_rng(order * 8 + bos * 4 + eos * 2 + unk)
    backoffs = absent = 0
    for _ in range(3):
        grams, text = lm_ref.random_arpa(rng, V, order, 7, 30, bos, eos, unk)
        lm = _lm(text, V)
        assert lm.order == max(len(g) for g in grams) and lm.has_bos == bos and lm.has_eos == eos
        assert (lm.start != 0) == any(len(g) == 2 and g[0] == "<s>" for g in grams)
        assert bool((lm.bo_state[1:] < np.arange(1, lm.n_states)).all())
        for _ in range(40):
            y = [int(t) for t in rng.integers(0, V, int(rng.integers(0, 9)))]
            absent += sum(1 for t in y if (t,) not in grams)
            for use_eos in (False, True):
                want = lm_ref.arpa_score(grams, y, eos=use_eos)
                assert lm.score(y, eos=use_eos) == pytest.approx(want, abs=1e-6, rel=1e-6), (y, use_eos)
            backoffs += lm.walk(y, detail=True)[2]
    assert absent > 0 and (order == 1 or backoffs > 0)


def test_unk_logp_argument_and_units(tmp_path):
    from m3asr.lm import NgramLm, read_arpa
    text = "\\data\\\nngram 1=3\nngram 2=1\n\n\\1-grams:\n-1.0\ta\t-0.5\n-0.7\tb\n-99\t<s>\t-0.25\n\n\\2-grams:\n-0.3\t<s> a\n\n\\end\\\n"
    units = {"a": 3, "b": 1, "c": 5}
    lm = NgramLm.from_arpa(text, units)
    assert lm.vocab_size == 6 and lm.unk_logp == pytest.approx(math.log(1e-10), rel=1e-6)
    ln10 = math.log(10.0)
    assert lm.score([3]) == pytest.approx(-0.3 * ln10, rel=1e-6)
    assert lm.score([1]) == pytest.approx((-0.25 - 0.7) * ln10, rel=1e-6)          # <s> backs off to the unigram
    assert lm.score([5]) == pytest.approx(-0.25 * ln10 + math.log(1e-10), rel=1e-6)
    assert NgramLm.from_arpa(text, units, unk_logp=-7.0).score([5]) == pytest.approx(-0.25 * ln10 - 7.0, rel=1e-6)
    f, u = tmp_path / "lm.arpa", tmp_path / "units.txt"
    f.write_text(text)
    u.write_text("a 3\nb 1\nc 5\n")
    again = NgramLm.from_arpa(str(f), str(u))
    assert np.array_equal(again.image, lm.image)
    with pytest.raises(ValueError, match="not in the units"):
        read_arpa(text, {"a": 3})
    with pytest.raises(ValueError, match="blank"):
        NgramLm.from_arpa(text, {"a": 0, "b": 1})
    with pytest.raises(ValueError, match="promises"):
        read_arpa(text.replace("ngram 1=3", "ngram 1=4"), units)


# ------------------------------------------------------------------------------------------------ 2. a normalised LM
def _absolute_discounting(corpus, V, D=0.5):
    """Interpolated absolute discounting, order 3, written as a back-off model: an n-gram that was seen holds its full
    interpolated probability, the context's back-off weight is the mass the discount freed.  Every token 1 .. V-1 and </s>
    can be predicted (the unigrams are interpolated with the uniform distribution)."""
    counts = [Counter(), Counter(), Counter()]
    for sent in corpus:
        words = ["<s>"] + list(sent) + ["</s>"]
        for i in range(1, len(words)):
            for n in range(3):
                if i - n >= 0:
                    counts[n][tuple(words[i - n:i + 1])] += 1
    vocab = list(range(1, V)) + ["</s>"]
    total = sum(counts[0].values())
    lam0 = D * len(counts[0]) / total
    p1 = {w: max(counts[0][(w,)] - D, 0.0) / total + lam0 / len(vocab) for w in vocab}
    prob = {(w,): p for w, p in p1.items()}
    bow = {}
    for n in (1, 2):
        ctx_total, ctx_types = Counter(), Counter()
        for g, c in counts[n].items():
            ctx_total[g[:-1]] += c
            ctx_types[g[:-1]] += 1
        for h in ctx_total:
            bow[h] = D * ctx_types[h] / ctx_total[h]
        for g, c in counts[n].items():
            h = g[:-1]
            lower = prob.get(g[1:])
            if lower is None:                                     # the lower order backs off itself
                lower = bow.get(g[1:-1], 1.0) * prob[g[2:]]
            prob[g] = (c - D) / ctx_total[h] + bow[h] * lower
    grams = {g: (math.log10(p), math.log10(bow[g]) if g in bow else 0.0) for g, p in prob.items()}
    grams[("<s>",)] = (-99.0, math.log10(bow[("<s>",)]))
    return grams


def test_compiled_automaton_of_a_normalised_lm_sums_to_one():
    V = 7
    rng = np.random.default_rng(4)
    corpus = [[int(t) for t in rng.integers(1, V, int(rng.integers(1, 7)))] for _ in range(60)]
    grams = _absolute_discounting(corpus, V)
    text = lm_ref.arpa_text({g: (round(lp, 7), round(b, 7)) for g, (lp, b) in grams.items()})
    lm = _lm(text, V)
    assert lm.order == 3 and lm.start != 0
    seen, todo = {lm.start}, [lm.start]
    while todo:
        s = todo.pop()
        total = math.exp(float(lm.final[s]))
        for tok in range(V):
            lp, nxt, _ = lm.step(s, tok)
            total += math.exp(lp)
            if tok != 0 and nxt not in seen:
                seen.add(nxt)
                todo.append(nxt)
        assert total == pytest.approx(1.0, abs=1e-5), (s, total)
    assert len(seen) > 10


# ------------------------------------------------------------------------------------------------ 3. the fused host search
def _case_large():
    V, T, beam, order = 1434, 50, 10, 3
    rng = np.random.default_rng(31)
    x = rng.normal(0, 2.0, (T, V)).astype(np.float32)
    x[::4, 0] += 4.0
    path = ref.ctc_greedy_search(x[None], [T], 0)[0]
    return x, V, beam, order, path, rng


def _case_small():
    V, T, beam, order = 5, 300, 4, 4
    rng = np.random.default_rng(32)
    return rng.normal(0, 1.5, (T, V)).astype(np.float32), V, beam, order, [1, 2, 3, 1, 2, 4, 4, 3], rng


def _same(got, want, tol=1e-6):
    assert [h[0] for h in got] == [h[0] for h in want]
    for i in (1, 2, 3):
        np.testing.assert_allclose([h[i] for h in got], [h[i] for h in want], rtol=tol, atol=tol)
    assert [h[4] for h in got] == [h[4] for h in want]


@pytest.mark.parametrize("case", [_case_large, _case_small])
@pytest.mark.parametrize("with_graph", [False, True])
def test_host_lm_search_matches_python_fused_search(case, with_graph):
    from m3asr import ops
    from m3asr.context import ContextGraph, ContextSet
    x, V, beam, order, path, rng = case()
    _, text = lm_ref.arpa_around(path, V, order, rng)
    lm = _lm(text, V)
    graph = image = None
    if with_graph:
        graph = ContextGraph([path[2:5], path[1:3]], V, score=1.5)
        image = ContextSet([graph]).image
    lp, ix = ref.topk_desc(ref.log_softmax(x), min(beam, V))
    alpha, beta = 0.7, 0.4
    for use_eos in (False, True):
        got = ops.ctc_prefix_beam_search_lm_host(lp, ix, beam, 0, image, 0, lm.image, alpha, beta, use_eos)
        want = lm_ref.fused_beam_search(lp, ix, beam, 0, graph, lm.walk, lambda s: float(lm.final[s]), alpha, beta, use_eos)
        _same(got, want)
    assert all(h[3] != 0.0 for h in got if h[0]), "the case does not exercise the LM"
    assert sum(lm.walk(h[0], detail=True)[2] for h in got) > 0, "no back-off step in this case"
    plain = ops.ctc_prefix_beam_search_ctx_host(lp, ix, beam, 0, image, 0)
    assert [h[0] for h in got] != [h[0] for h in plain], "the LM changes nothing in this case"
    if with_graph:
        assert any(h[2] != 0.0 for h in got), "the case does not exercise the bonus"


# ------------------------------------------------------------------------------------------------ 4. no LM, or no weight
@pytest.mark.parametrize("T,V,beam,blank", [(50, 1434, 10, 0), (300, 5, 4, 0), (70, 30, 6, 7), (1, 3, 3, 0)])
def test_null_lm_or_zero_weights_are_the_ctx_routine(T, V, beam, blank):
    from m3asr import ops
    from m3asr.context import ContextGraph, ContextSet
    from m3asr.lm import NgramLm
    rng = np.random.default_rng(T + V)
    x = rng.normal(0, 2.0, (T, V)).astype(np.float32)
    x[::5, blank] += 3.0
    lp, ix = ref.topk_desc(ref.log_softmax(x), min(beam, V))
    toks = [t for t in range(V) if t != blank]
    image = ContextSet([ContextGraph([toks[:2], toks[1:2]], V, score=2.0, blank=blank)]).image
    grams, _ = lm_ref.random_arpa(rng, V, 3, 8, 40, blank=blank)
    lm = NgramLm.from_arpa(lm_ref.arpa_text(grams), None, blank=blank, vocab_size=V)
    for img in (None, image):
        want = ops.ctc_prefix_beam_search_ctx_host(lp, ix, beam, blank, img, 0)
        null = ops.ctc_prefix_beam_search_lm_host(lp, ix, beam, blank, img, 0, None, 0.9, 0.3, True)
        assert [(h[0], h[1], h[2], h[4]) for h in null] == want   # float equality, not a tolerance
        assert all(h[3] == 0.0 for h in null)
        zero = ops.ctc_prefix_beam_search_lm_host(lp, ix, beam, blank, img, 0, lm.image, 0.0, 0.0, False)
        assert [(h[0], h[1], h[2], h[4]) for h in zero] == want
        if T > 1:
            assert any(h[3] != 0.0 for h in zero)                 # the LM still ran: hyp_lm is reported


# ------------------------------------------------------------------------------------------------ 5. by hand
def test_hand_built_case_flips_with_the_lm_weight():
    from m3asr import ops
    V = 6
    # every frame but one is all but certain; frame 4 has tokens 4 and 3 tied within 0.1 nat, and the LM prefers 3 by > 1 nat
    p = np.full((6, V), 1e-7)
    for t, tok in enumerate([1, 0, 2, 0, None, 0]):
        if tok is None:
            p[t, 4], p[t, 3] = 0.51, 0.49 - 4e-7
        else:
            p[t, tok] = 1.0 - 5e-7
    assert 0 < math.log(0.51 / 0.49) < 0.1
    text = ("\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-1.0\t1\t-0.2\n-1.0\t2\t-0.2\n-1.0\t3\n-1.0\t4\n-1.0\t5\n\n"
            "\\2-grams:\n-0.2\t1 2\n-0.1\t2 3\n-1.0\t2 4\n\n\\end\\\n")
    lm = _lm(text, V)
    gap = lm.score([1, 2, 3]) - lm.score([1, 2, 4])
    assert gap == pytest.approx(0.9 * math.log(10.0), rel=1e-6) and gap > 1.0
    lp, ix = ref.topk_desc(np.log(p).astype(np.float32), V)
    off = ops.ctc_prefix_beam_search_lm_host(lp, ix, 6, 0, None, 0, lm.image, 0.0, 0.0, False)
    on = ops.ctc_prefix_beam_search_lm_host(lp, ix, 6, 0, None, 0, lm.image, 1.0, 0.0, False)
    assert off[0][0] == (1, 2, 4) and off[1][0] == (1, 2, 3) and 0 < off[0][1] - off[1][1] < 0.1
    assert on[0][0] == (1, 2, 3) and on[1][0] == (1, 2, 4)
    ctc = {h[0]: h[1] for h in off}
    for h in on[:2]:
        assert h[1] == pytest.approx(ctc[h[0]], abs=1e-6)         # hyp_score stays the CTC score
        assert h[3] == pytest.approx(lm.score(h[0]), abs=1e-5)


# ------------------------------------------------------------------------------------------------ 6. validate
def _small_lm():
    rng = np.random.default_rng(9)
    grams, text = lm_ref.random_arpa(rng, 10, 3, 6, 25)
    lm = _lm(text, 10)
    assert lm.n_states > 3 and lm.n_arcs > 6
    return lm


def _mutations(lm):
    """(what the message must name, position in the image, value): one mutation per check of m3_ctc_lm_validate"""
    img = lm.image
    off = {name: int(img[8 + i]) for i, name in enumerate(("uni_logp", "uni_next", "arc_begin", "arc_tok", "arc_next", "arc_logp",
                                                          "bo_state", "bo_weight", "final"))}
    nan = int(np.float32(np.nan).view(np.int32))
    inf = int(np.float32(np.inf).view(np.int32))
    s = next(s for s in range(1, lm.n_states - 1) if lm.arc_begin[s + 1] - lm.arc_begin[s] >= 2)    # a state with two arcs
    a = int(lm.arc_begin[s])
    deep = any(lm.bo_state[s] != 0 for s in range(1, lm.n_states))          # a chain of two levels
    return [
        ("not an LM image", 0, 0x5843334D),
        ("version", 1, 2),
        ("words", 17, img.size + 1),
        ("order", 3, 9),
        ("order", 4, 0),                                          # n_states
        ("order", 6, lm.n_states),                                # start
        ("order", 8 + 5, img.size - 1),                           # arc_logp runs off the image
        ("unk_logp", 7, nan),
        ("uni_logp", off["uni_logp"] + 2, inf),
        ("uni_next", off["uni_next"] + 2, lm.n_states),
        ("arc_begin", off["arc_begin"] + 1, 1),
        ("arc_begin", off["arc_begin"] + lm.n_states, lm.n_arcs - 1),
        ("monotone", off["arc_begin"] + s + 1, a - 1 if a > 0 else lm.n_arcs + 1),
        ("arc_tok", off["arc_tok"] + a, -1),
        ("arc_tok", off["arc_tok"] + a, lm.vocab_size),
        ("not above", off["arc_tok"] + a + 1, int(lm.arc_tok[a])),
        ("arc_next", off["arc_next"] + a, lm.n_states),
        ("arc_next", off["arc_next"] + a, -1),
        ("arc_logp", off["arc_logp"] + a, nan),
        ("bo_state", off["bo_state"] + s, s),
        ("bo_state", off["bo_state"] + 0, 1),
        ("bo_state", off["bo_state"] + s, -1),
        ("bo_weight", off["bo_weight"] + s, inf),
        ("final", off["final"] + s, nan),
        ("levels", 3, 2) if lm.order == 3 and deep else None,
    ]


def test_validate_rejects_each_malformed_table():
    from m3asr import ops
    from m3asr._lib import M3Error
    lm = _small_lm()
    ops.ctc_lm_validate(lm.image, lm.vocab_size)
    with pytest.raises(M3Error, match="V ="):
        ops.ctc_lm_validate(lm.image, lm.vocab_size + 1)
    with pytest.raises(M3Error):
        ops.ctc_lm_validate(lm.image[:-1], lm.vocab_size)
    with pytest.raises(M3Error):
        ops.ctc_lm_validate(lm.image[:10], lm.vocab_size)
    for m in _mutations(lm):
        if m is None:
            continue
        what, pos, value = m
        img = lm.image.copy()
        assert int(img[pos]) != value, m
        img[pos] = value
        with pytest.raises(M3Error, match=what):
            ops.ctc_lm_validate(img, lm.vocab_size)
    with pytest.raises(M3Error, match="arc_next"):                # the host search validates what it is handed
        img = lm.image.copy()
        img[int(img[8 + 4])] = lm.n_states
        ops.ctc_prefix_beam_search_lm_host(np.zeros((2, 2), np.float32), np.array([[0, 1], [1, 0]], np.int32), 2, 0, None, 0, img)


# ------------------------------------------------------------------------------------------------ 7. save / load
def test_save_load_round_trip(tmp_path):
    from m3asr.lm import NgramLm
    lm = _small_lm()
    path = str(tmp_path / "lm.npy")
    lm.save(path)
    back = NgramLm.load(path)
    assert np.array_equal(back.image, lm.image) and back.image.dtype == np.int32
    for name in ("vocab_size", "order", "n_states", "n_arcs", "start", "unk_logp"):
        assert getattr(back, name) == getattr(lm, name), name
    rng = np.random.default_rng(1)
    for _ in range(20):
        y = [int(t) for t in rng.integers(0, 10, 6)]
        assert back.walk(y) == lm.walk(y) and back.score(y, eos=True) == lm.score(y, eos=True)
    np.save(path, np.arange(30, dtype=np.int32))
    with pytest.raises(ValueError):
        NgramLm.load(path)


# ------------------------------------------------------------------------------------------------ 8. the ABI
NEW_EXPORTS = ["m3_ctc_beam_lm_advance", "m3_ctc_beam_lm_nbest", "m3_ctc_beam_lm_reset", "m3_ctc_beam_lm_reset_slots",
               "m3_ctc_beam_lm_state_size", "m3_ctc_lm_validate", "m3_ctc_prefix_beam_search_lm"]


def test_new_exports_and_unchanged_abi_version():
    from m3asr import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m3asr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(m3_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(n for n in declared if "_lm" in n) == NEW_EXPORTS
    assert _lib.load().m3_abi_version() == 10
    # the state: the biased search's layout, then the LM blocks
    from m3asr import ops
    desc = ops.ctc_beam_desc(3, 4, 10, 0)
    assert ops.ctc_beam_lm_state_size(desc) > ops.ctc_beam_ctx_state_size(desc) > ops.ctc_beam_state_size(desc)


def test_kenlm_probe_is_an_import_attempt():
    from m3asr import lm
    assert lm.have_kenlm() in (True, False)
