"""CPU tier of the WFST decoding path: the graph image and its compilers (m3asr.wfst), the C validator (m3_wfst_validate) and
the host restatement of the search contract (tests/wfst_ref.py), which the GPU tier compares the device search against.

The restatement itself is pinned against an exhaustive float32 trellis on graphs of at most 12 states, with no beam: the
best final cost must have the same bits and the words (and their frames) must be the same.
"""
import itertools
import math

import numpy as np
import pytest

import wfst_cases as WC
import wfst_ref as R
from m3asr import _lib, ops
from m3asr.wfst import DecodingGraph, MAGIC, read_lexicon

INF = math.inf


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------------------------------- restatement == trellis
@pytest.mark.parametrize("seed", range(40))
def test_restatement_equals_exhaustive_trellis(seed):
    case = WC.tiny_case(seed)
    g, logp = case["graph"], case["logp"]
    assert g.n_states <= 12
    got, _ = R.search(g, logp, INF, g.n_states)
    cost, words, frames = R.trellis(g, logp)
    if cost is None:
        assert got["reached_final"] == 0
        return
    assert got["reached_final"] == 1 and got["status"] == 0
    assert _bits(got["cost"]) == _bits(cost)
    assert got["words"] == words and got["frames"] == frames


def test_trellis_cases_are_not_trivial():
    outs = [R.trellis(c["graph"], c["logp"]) for c in map(WC.tiny_case, range(40))]
    assert sum(o[0] is not None for o in outs) >= 20 and sum(len(o[1]) >= 2 for o in outs) >= 10
    assert any(c["graph"].n_levels >= 3 for c in map(WC.tiny_case, range(40)))


def test_random_cases_fire_every_mechanism():
    """The cases the GPU tier runs: the beam cut, the max_active cut decided by the state id at a cost tie, an epsilon winner
    over an emitting candidate and a dead search each decide something in at least one of them."""
    fired, settings = set(), set()
    for seed in WC.RANDOM_SEEDS:
        c = WC.random_case(seed)
        g = c["graph"]
        assert 6 <= g.n_states <= 40 and 3 <= g.vocab_size <= 6 and 1 <= len(c["logp"]) <= 60 and g.n_levels <= 6
        _, r = R.search(g, c["logp"], c["beam"], c["max_active"])
        fired |= r.fired
        settings.add((c["beam"], c["max_active"] if c["max_active"] != g.n_states else None))
    assert {"beam", "max_active_tie", "eps_over_emit", "dead"} <= fired, fired
    assert settings == set(itertools.product(WC.BEAMS, WC.MAX_ACTIVE))
    assert any(WC.random_case(s)["graph"].n_levels >= 5 for s in WC.RANDOM_SEEDS)


def test_restatement_is_chunk_invariant_and_soft_on_capacities():
    c = WC.random_case(4)
    g, logp = c["graph"], c["logp"]
    whole, _ = R.search(g, logp, 4.0, 5)
    r = R.RefSearch(g, 4.0, 5)
    for i in range(0, len(logp), 7):
        r.advance(logp[i:i + 7])
    assert r.result() == whole
    assert R.search(g, logp, 4.0, 5, max_frames=len(logp) - 1)[0]["status"] == R.MAX_FRAMES
    assert R.search(g, logp, 4.0, 5, record_cap=1)[0]["n_words"] == -1
    assert R.search(g, logp, INF, g.n_states, token_cap=2)[0]["status"] & R.TOKEN_CAP


# ---------------------------------------------------------------------------------------- the image and the compilers
def test_fst_text_round_trip_and_eps_level():
    for seed in (0, 5, 11, 17):
        g = WC.random_case(seed)["graph"]
        h = DecodingGraph.from_fst_text(g.to_fst_text(), g.vocab_size)
        assert np.array_equal(h.image, g.image)
        g.validate()
        # eps_level against a brute-force longest path over the epsilon-input arcs
        src = R.arc_sources(g)
        eps = [(int(src[a]), int(g.arc_dst[a])) for a in range(g.n_arcs) if g.arc_ilabel[a] == 0]

        def longest(s, seen=()):
            assert s not in seen
            return max([1 + longest(p, seen + (s,)) for p, d in eps if d == s], default=0)

        assert [longest(s) for s in range(g.n_states)] == g.eps_level.tolist()
        assert g.n_levels == int(g.eps_level.max()) + 1


def test_fst_text_symbols_start_state_and_defaults(tmp_path):
    text = "3 1 a X 0.5\n1 3 <eps> <eps>\n1 2 b <eps> -0.0\n2\n3 1.5\n"
    isym, osym = {"<eps>": 0, "a": 1, "b": 2}, {"<eps>": 0, "X": 7}
    g = DecodingGraph.from_fst_text(text, 2, isym, osym)
    assert g.start == 3 and g.n_states == 4 and g.n_arcs == 3
    assert g.final.tolist() == [INF, INF, 0.0, 1.5]
    a = int(g.arc_begin[1])                                   # state 1: the emitting arc first, then the epsilon one
    assert g.arc_ilabel[a:a + 2].tolist() == [2, 0] and g.eps_begin[1] == a + 1
    assert _bits(g.arc_weight[a]) == 0                         # -0.0 is stored as +0.0
    assert g.eps_level.tolist() == [0, 0, 0, 1] and g.n_levels == 2
    p = tmp_path / "g.txt"
    p.write_text(text)
    sp = tmp_path / "isym.txt"
    sp.write_text("<eps> 0\na 1\nb 2\n")
    assert np.array_equal(DecodingGraph.from_fst_text(str(p), 2, str(sp), osym).image, g.image)
    with pytest.raises(ValueError, match="not in the symbol table"):
        DecodingGraph.from_fst_text("0 1 zz X\n1\n", 2, isym, osym)


def test_save_load_round_trip(tmp_path):
    g = WC.random_case(2)["graph"]
    g.save(tmp_path / "g.npy")
    h = DecodingGraph.load(tmp_path / "g.npy")
    assert np.array_equal(h.image, g.image) and h.n_levels == g.n_levels and h.start == g.start
    for name in ("arc_begin", "eps_begin", "arc_ilabel", "arc_olabel", "arc_dst", "arc_weight", "final", "eps_level"):
        assert np.array_equal(getattr(h, name), getattr(g, name)), name
    assert int(g.image[0]) == MAGIC and g.image[:4].tobytes()[:4] == b"M3FS"
    np.save(tmp_path / "bad.npy", np.zeros(30, dtype=np.int32))
    with pytest.raises(ValueError, match="not a graph image"):
        DecodingGraph.load(tmp_path / "bad.npy")


# ---------------------------------------------------------------------------------------- from_lexicon
def _collapse(seq, blank):
    out = []
    for i, t in enumerate(seq):
        if t != blank and (i == 0 or t != seq[i - 1]):
            out.append(t)
    return tuple(out)


def _segment_cost(tokens, entries):
    """The smallest word-cost sum over the segmentations of `tokens` into lexicon entries (None: there is none)."""
    best = {0: 0.0}
    for i in range(len(tokens)):
        if i in best:
            for pron, cost in entries:
                if tokens[i:i + len(pron)] == pron:
                    j = i + len(pron)
                    best[j] = min(best.get(j, INF), best[i] + cost)
    return best.get(len(tokens))


LEXICONS = [
    (3, {1: [1], 2: [1, 2]}, {1: 0.5, 2: 0.25}),                                  # a shared prefix
    (4, {1: [1, 2], 2: [2, 3], 3: [1, 2, 3]}, {1: 1.0, 2: 0.5, 3: 2.0}),          # word 1 ends in the token word 2 starts with
    (3, {1: [2, 2], 2: [2], 3: [1, 2], 4: [[1], [2, 1]]}, None),                  # a doubled token, two entries for one word
    (4, WC.TOY_LEXICON, {1: 0.25, 2: 0.5, 3: 0.75, 4: 1.0}),
]


@pytest.mark.parametrize("V,lexicon,costs", LEXICONS)
def test_from_lexicon_accepts_exactly_the_ctc_alignments(V, lexicon, costs):
    g = DecodingGraph.from_lexicon(lexicon, V, blank=0, word_costs=costs).validate()
    entries = []
    for wid, prons in lexicon.items():
        for pron in (prons if isinstance(prons[0], list) else [prons]):
            entries.append((tuple(pron), 0.0 if costs is None else costs[wid]))
    prons_of = {w: [tuple(q) for q in (p if isinstance(p[0], list) else [p])] for w, p in lexicon.items()}
    n_accept = 0
    for n in range(7):
        for seq in itertools.product(range(V), repeat=n):
            want = _segment_cost(_collapse(seq, 0), entries)
            got = R.accepts(g, [t + 1 for t in seq])
            assert (got is None) == (want is None), seq
            if want is not None:
                n_accept += 1
                assert got[0] == want, seq
                # every word once: some entry of each output word, in order, spells the collapsed sequence
                assert any(sum(p, ()) == _collapse(seq, 0) for p in itertools.product(*[prons_of[w] for w in got[1]])), (seq, got)
    assert n_accept > 50


def test_from_lexicon_through_the_search_and_the_lexicon_file(tmp_path):
    g = DecodingGraph.from_lexicon(WC.TOY_LEXICON, 4, word_costs={2: 0.5})
    # "1 2 3 | 3 3 | 2 1" with blanks and repeats: word 2, then word 3 (a blank between the 3s), then word 4
    ali = [0, 1, 1, 2, 3, 0, 3, 3, 0, 3, 0, 0, 2, 2, 1, 0]
    logp = np.log(np.exp(WC.peaked_logits(ali, 4)) / np.exp(WC.peaked_logits(ali, 4)).sum(-1, keepdims=True)).astype(np.float32)
    got, _ = R.search(g, logp, 8.0, 50)
    assert got["words"] == [2, 3, 4] and got["reached_final"] == 1
    assert got["frames"] == sorted(got["frames"]) and got["frames"][0] >= 4
    p = tmp_path / "lex.txt"
    p.write_text("ab 1 2\nabc 1 2 3\ncc 3 3\nba 2 1\nab 2 2\n")
    lex, words = read_lexicon(str(p))
    assert words == ["ab", "abc", "cc", "ba"] and lex[1] == [[1, 2], [2, 2]] and lex[4] == [[2, 1]]
    with pytest.raises(ValueError, match="blank"):
        DecodingGraph.from_lexicon({1: [0, 1]}, 4)
    with pytest.raises(ValueError, match="empty"):
        DecodingGraph.from_lexicon({}, 4)


# ---------------------------------------------------------------------------------------- refusals
def _image():
    return WC.random_case(5)["graph"]


def _refused(img, V, match):
    with pytest.raises(_lib.M3Error, match=match):
        ops.wfst_validate(img, V)


def _table(g, img, name):
    i = ("arc_begin", "eps_begin", "arc_ilabel", "arc_olabel", "arc_dst", "arc_weight", "final", "eps_level").index(name)
    off = int(img[8 + i])
    return img[off:off + len(getattr(g, name))]


def test_validator_refusals():
    g = _image()
    V = g.vocab_size
    ops.wfst_validate(g.image, V)
    assert any(g.arc_ilabel == 0) and g.n_levels >= 2

    def mutated(name, index, value):
        img = g.image.copy()
        t = _table(g, img, name)
        (t.view(np.float32) if isinstance(value, float) else t)[index] = value
        return img

    _refused(mutated("arc_dst", 0, g.n_states), V, "dst = %d outside" % g.n_states)
    _refused(mutated("arc_dst", 1, -1), V, "dst = -1 outside")
    a_emit = int(np.flatnonzero(g.arc_ilabel != 0)[-1])
    _refused(mutated("arc_ilabel", a_emit, V + 1), V, "ilabel = %d outside" % (V + 1))
    _refused(mutated("arc_weight", 0, float("nan")), V, "weight is not finite")
    _refused(mutated("arc_weight", 0, float("inf")), V, "weight is not finite")
    _refused(mutated("arc_weight", 0, -0.0), V, "weight is -0.0")
    _refused(mutated("final", 0, float("nan")), V, r"final\[0\] is NaN")
    s = int(np.argmax(g.eps_level))
    _refused(mutated("eps_level", s, int(g.eps_level[s]) - 1), V, r"eps_level\[%d\]" % s)
    img = g.image.copy()
    _table(g, img, "final").view(np.float32)[:] = np.inf
    _refused(img, V, "no final state")
    img = g.image.copy()
    _table(g, img, "arc_begin")[1] = g.n_arcs + 1
    _refused(img, V, "arc_begin")
    img = g.image.copy()
    img[8] = img[16] - 2
    _refused(img, V, "table outside the image")
    _refused(g.image, V + 1, "built for V")
    _refused(g.image[:-1], V, "words")
    for word, text in ((3, "n_states"), (6, "n_levels")):
        img = g.image.copy()
        img[word] = (1 << 26) + 1 if word == 3 else 65
        _refused(img, V, text)
    _refused(np.zeros(10, dtype=np.int32), V, "bytes")


def test_epsilon_cycle_is_named_by_compiler_and_validator():
    text = "0 1 1 0\n1 2 0 0\n2 3 0 0\n3 1 0 0\n3 4 0 0\n4\n"                     # 1 -> 2 -> 3 -> 1 by epsilons; 4 hangs off it
    with pytest.raises(ValueError, match=r"cycle through state [123]\b"):
        DecodingGraph.from_fst_text(text, 2)
    # the same graph as an image: build the acyclic one, then turn the arc 3 -> 4 ... into 3 -> 1 by hand
    g = DecodingGraph.from_fst_text("0 1 1 0\n1 2 0 0\n2 3 0 0\n3 4 0 0\n3 4 0 0 1\n4\n", 2)
    img = g.image.copy()
    dst = _table(g, img, "arc_dst")
    dst[int(g.arc_begin[3])] = 1
    _refused(img, 2, r"cycle through state [123]\b")


def test_compiler_refusals():
    with pytest.raises(ValueError, match="ilabel > V"):
        DecodingGraph.from_fst_text("0 1 3 0\n1\n", 2)
    with pytest.raises(ValueError, match="not finite"):
        DecodingGraph.from_fst_text("0 1 1 0 inf\n1\n", 2)
    with pytest.raises(ValueError, match="no final state"):
        DecodingGraph.from_fst_text("0 1 1 0\n", 2)
    with pytest.raises(ValueError, match="NaN"):
        DecodingGraph.from_fst_text("0 1 1 0\n1 nan\n", 2)
    chain = "".join("%d %d 0 0\n" % (i, i + 1) for i in range(64)) + "64\n"
    with pytest.raises(ValueError, match="n_levels"):
        DecodingGraph.from_fst_text(chain, 2)
    assert DecodingGraph.from_fst_text("".join("%d %d 0 0\n" % (i, i + 1) for i in range(63)) + "63\n", 2).validate().n_levels == 64


def test_state_size_and_descriptor_checks():
    d = _lib.WfstSearchDesc(2, 100, 500, 1000, 7000, 1000, 3, 1434, 16.0, 1.0)
    n = ops.wfst_search_state_size(d)
    assert n % 512 == 0 and n // 2 >= 24 * 1000 + 4 * (2 * 500 + 3 * 500 + 3 * 1000)
    big = _lib.WfstSearchDesc(1, 100, 500, 1000, 7000, 10_000_000, 3, 1434, 16.0, 1.0)
    assert 240e6 <= ops.wfst_search_state_size(big) <= 241e6                       # 24 bytes per graph state
    for field, value in (("beam", 0.0), ("beam", float("nan")), ("max_active", 0), ("token_cap", 0), ("record_cap", 0),
                         ("n_levels", 65), ("V", 20000), ("acoustic_scale", float("inf")), ("n_states", 0), ("max_frames", 0)):
        bad = _lib.WfstSearchDesc.from_buffer_copy(d)
        setattr(bad, field, value)
        with pytest.raises(_lib.M3Error, match=field if field != "V" else "V ="):
            ops.wfst_search_state_size(bad)
    inf_beam = _lib.WfstSearchDesc.from_buffer_copy(d)
    inf_beam.beam = INF
    assert ops.wfst_search_state_size(inf_beam) == n
