"""Hotword biasing of the CTC prefix beam search, host side: the phrase compiler (m3asr.context.ContextGraph / ContextSet),
the image check (m3_ctc_context_validate) and the biased host search (m3_ctc_prefix_beam_search_ctx), which is the
yardstick of the device search (tests/test_ctc_context_gpu.py).

Yardsticks here: worked examples; a brute-force substring count that knows nothing of tries or failure links; a pure-Python
biased prefix beam search (the structure of oracle.ctc_decode.prefix_beam_search_topk plus the ranking rule: prune by
log_add(pb, pnb) + bonus, report by log_add(pb, pnb) + final, both stable) on the same top-k pairs -- prefixes and order
identical, scores and bonus to 1e-6, the bound tests/test_ctc_beam_gpu.py uses between device and host.
"""
import numpy as np
import pytest

from oracle import ctc_decode as ref

W = 3.0


def _graph(phrases, V=16, w=W, blank=0):
    from m3asr.context import ContextGraph
    return ContextGraph(phrases, V, score=w, blank=blank)


# ------------------------------------------------------------------------------------------------ 1. worked examples
def test_worked_examples():
    g = _graph([[7, 8, 9]])
    assert [g.walk([7, 8, 9][:i])[1] for i in (1, 2, 3)] == [W, 2 * W, 3 * W]
    assert g.walk([7, 8, 9])[2] == 3 * W
    assert [g.walk([7, 8, 4][:i])[1] for i in (1, 2, 3)] == [W, 2 * W, 0.0]
    assert g.walk([7, 8, 4])[2] == 0.0
    assert g.walk([7, 8])[1:] == (2 * W, 0.0)                   # in state "7 8": bonus 2w, none of it final
    assert g.walk([])[0] == 0 and g.walk([7, 8, 4])[0] == 0
    g = _graph([[1, 2], [1, 2, 3]])
    assert g.walk([1, 2])[2] == 2 * W and g.walk([1, 2, 3])[2] == 3 * W    # the longer phrase earns its additional token
    g = _graph([[1, 2, 3, 4], [2, 3]])
    assert g.walk([1, 2, 3, 5])[2] == 2 * W
    assert g.walk([1, 2, 3])[1:] == (5 * W, 2 * W)              # "2 3" is complete inside the partial "1 2 3"
    assert g.walk([1, 2, 3, 4])[2] == 6 * W


# ------------------------------------------------------------------------------------------------ 2. property
def _prefix_free_sets(rng, n_sets, V):
    """Random phrase sets over tokens 1 .. V-1 in which no phrase is a prefix of another (equal phrases included): a
    candidate that is a prefix of, or has as a prefix, a phrase already chosen is redrawn, not dropped after the fact."""
    sets = []
    while len(sets) < n_sets:
        want, chosen = int(rng.integers(1, 6)), []
        for _ in range(200):
            if len(chosen) == want:
                break
            p = tuple(int(t) for t in rng.integers(1, V, int(rng.integers(1, 5))))
            if all(p[:len(q)] != q and q[:len(p)] != p for q in chosen):
                chosen.append(p)
        if len(chosen) == want:
            sets.append(chosen)
    return sets


def test_final_is_the_brute_force_occurrence_count():
    V, w = 6, 1.5
    rng = np.random.default_rng(5)
    sets = _prefix_free_sets(rng, 40, V)
    assert len(sets) == 40
    longest = 0
    for phrases in sets:
        for a in phrases:                                         # the generator's promise, checked
            for b in phrases:
                assert a is b or a[:len(b)] != b
        longest = max(longest, max(len(p) for p in phrases))
        g = _graph([list(p) for p in phrases], V, w)
        for _ in range(6):
            y = [int(t) for t in rng.integers(0, V, 40)]
            for n in range(len(y) + 1):
                want = sum(len(p) for p in phrases for e in range(len(p), n + 1) if tuple(y[e - len(p):e]) == p)
                assert g.walk(y[:n])[2] == w * want, (phrases, y[:n])
    assert longest >= 3


# ------------------------------------------------------------------------------------------------ 3. tables, errors, validate
def test_tables_and_rejections():
    from m3asr import ops
    from m3asr._lib import M3Error
    from m3asr.context import ContextGraph, ContextSet
    V = 12
    phrases = [[3, 4, 5], [4, 5], [9], [3, 9, 9, 4]]
    g = ContextGraph(phrases, V, score=2.0, blank=0)
    assert g.next.shape == (g.n_states, g.A) == g.delta.shape and g.pot.shape == (g.n_states,) and g.cls.shape == (V,)
    assert g.next.dtype == np.int32 and g.cls.dtype == np.int32 and g.delta.dtype == np.float32 and g.pot.dtype == np.float32
    assert g.next.min() >= 0 and g.next.max() < g.n_states
    used = {t for p in phrases for t in p}
    assert {v for v in range(V) if g.cls[v] != 0} == used
    assert sorted(int(g.cls[v]) for v in used) == list(range(1, g.A)) and g.A == len(used) + 1
    assert (g.next[:, 0] == 0).all()                              # a token in no phrase leads back to the start
    for bad in ([[3, V]], [[-1]], [[0, 3]], [[]], [[3, 4], [3, 4]]):
        with pytest.raises(ValueError):
            ContextGraph(bad, V, blank=0)
    with pytest.raises(ValueError):
        ContextGraph([[7]], V, blank=7)
    # the image: what the library accepts, and a corrupted next entry
    cs = ContextSet([g, ContextGraph([[1, 2]], V)])
    assert len(cs) == 2 and cs.dev is None
    ops.ctc_context_validate(cs.image, V)
    ContextSet([], vocab_size=V)                                  # G = 0 is a valid set
    with pytest.raises(M3Error):
        ops.ctc_context_validate(cs.image, V + 1)
    off_next = int(cs.image[4 + 3])
    for bad_value in (g.n_states, -1, 1 << 30):
        img = cs.image.copy()
        img[off_next + g.A + 1] = bad_value
        with pytest.raises(M3Error, match="next"):
            ops.ctc_context_validate(img, V)
    img = cs.image.copy()
    img[int(cs.image[4 + 2]) + 3] = g.A                           # cls[3] one past the last column
    with pytest.raises(M3Error, match="cls"):
        ops.ctc_context_validate(img, V)
    img = cs.image.copy()
    img[4 + 8 + 3] = img.size - 1                                 # graph 1's next table runs off the image
    with pytest.raises(M3Error):
        ops.ctc_context_validate(img, V)
    with pytest.raises(M3Error):
        ops.ctc_context_validate(cs.image[:-1], V)
    with pytest.raises(M3Error):                                  # and the host search validates what it is handed
        img = cs.image.copy()
        img[off_next] = g.n_states
        ops.ctc_prefix_beam_search_ctx_host(np.zeros((2, 2), np.float32), np.array([[0, 1], [1, 0]], np.int32), 2, 0, img, 0)


def test_read_phrases(tmp_path):
    from m3asr.context import read_phrases
    f = tmp_path / "words.txt"
    f.write_text("7 8 9\n\n# a comment\n  12\t4 \n")
    assert read_phrases(str(f)) == [[7, 8, 9], [12, 4]]
    f.write_text("7 eight\n")
    with pytest.raises(ValueError, match="words.txt:1"):
        read_phrases(str(f))


# ------------------------------------------------------------------------------------------------ 4. the biased host search
def _python_biased_search(top_logp, top_idx, beam, blank, graph):
    """prefix_beam_search_topk with the biased ranking; (state, bonus, final) of a prefix come from graph.walk."""
    NEG = ref.NEG_INF
    walk = {}

    def ctx(prefix):
        if prefix not in walk:
            walk[prefix] = graph.walk(prefix) if graph is not None else (0, 0.0, 0.0)
        return walk[prefix]

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
        ranked = sorted(grown.items(), key=lambda kv: ref.log_add(*kv[1]) + ctx(kv[0])[1], reverse=True)
        beams = dict(ranked[:beam])
    out = [(p, ref.log_add(*v), ctx(p)[2], ctx(p)[0]) for p, v in beams.items()]
    return sorted(out, key=lambda h: h[1] + h[2], reverse=True)


def _same(got, want, tol=1e-6):
    assert [h[0] for h in got] == [h[0] for h in want]
    np.testing.assert_allclose([h[1] for h in got], [h[1] for h in want], rtol=tol, atol=tol)
    np.testing.assert_allclose([h[2] for h in got], [h[2] for h in want], rtol=tol, atol=tol)
    assert [h[3] for h in got] == [h[3] for h in want]


def _case_large():
    V, T, beam = 1434, 50, 10
    rng = np.random.default_rng(21)
    x = (rng.normal(0, 2.0, (T, V))).astype(np.float32)
    x[::4, 0] += 4.0
    path = ref.ctc_greedy_search(x[None], [T], 0)[0]
    phrases = set()
    while len(phrases) < 10:                                      # 10 from the greedy path ...
        n = int(rng.integers(2, 7))
        i = int(rng.integers(0, len(path) - n))
        phrases.add(tuple(path[i:i + n]))
    while len(phrases) < 20:                                      # ... and 10 from noise
        phrases.add(tuple(int(t) for t in rng.integers(1, V, int(rng.integers(2, 7)))))
    return x, [list(p) for p in sorted(phrases)], V, beam


def _case_small():
    V, T, beam = 5, 300, 4
    rng = np.random.default_rng(22)
    return rng.normal(0, 1.5, (T, V)).astype(np.float32), [[1, 2], [2, 3, 1], [3]], V, beam


@pytest.mark.parametrize("case", [_case_large, _case_small])
def test_host_ctx_search_matches_python_biased_search(case):
    from m3asr import ops
    from m3asr.context import ContextGraph, ContextSet
    x, phrases, V, beam = case()
    g = ContextGraph(phrases, V, score=W)
    other = ContextGraph([[1]], V, score=0.5)                     # the graph under test is not the first of its image
    cs = ContextSet([other, g])
    lp, ix = ref.topk_desc(ref.log_softmax(x), min(beam, V))
    got = ops.ctc_prefix_beam_search_ctx_host(lp, ix, beam, 0, cs.image, 1)
    want = _python_biased_search(lp, ix, beam, 0, g)
    _same(got, want)
    plain = ops.ctc_prefix_beam_search_host(lp, ix, beam, 0)
    assert any(h[2] != 0.0 for h in got), "the case does not exercise the bonus"
    assert [h[0] for h in got] != [p for p, _ in plain], "the bias changes nothing in this case"
    # graph -1 of a real image: unbiased
    assert [(h[0], h[1]) for h in ops.ctc_prefix_beam_search_ctx_host(lp, ix, beam, 0, cs.image, -1)] == plain
    with pytest.raises(ops._lib.M3Error):
        ops.ctc_prefix_beam_search_ctx_host(lp, ix, beam, 0, cs.image, 2)


# ------------------------------------------------------------------------------------------------ 5. null image
@pytest.mark.parametrize("T,V,beam,blank", [(50, 1434, 10, 0), (300, 5, 4, 0), (70, 30, 6, 7), (1, 3, 3, 0)])
def test_null_image_is_the_unbiased_routine(T, V, beam, blank):
    from m3asr import ops
    rng = np.random.default_rng(T + V)
    x = rng.normal(0, 2.0, (T, V)).astype(np.float32)
    x[::5, blank] += 3.0
    lp, ix = ref.topk_desc(ref.log_softmax(x), min(beam, V))
    got = ops.ctc_prefix_beam_search_ctx_host(lp, ix, beam, blank, None)
    want = ops.ctc_prefix_beam_search_host(lp, ix, beam, blank)
    assert [(h[0], h[1]) for h in got] == want                    # float equality, not a tolerance
    assert all(h[2] == 0.0 and h[3] == 0 for h in got)


# ------------------------------------------------------------------------------------------------ 6. StreamPool
class _StubDecoder:
    def __init__(self, context):
        self.context = context
        self.resets = []

    def reset(self, slots=None, graph_ids=None):
        self.resets.append((list(slots), None if graph_ids is None else list(graph_ids)))

    def finish(self, slots=None):
        return [[((), 0.0)] for _ in slots]


def test_stream_pool_routes_the_graph_id():
    from m3asr._lib import M3Error
    from m3asr.serve import StreamPool
    dec = _StubDecoder(context=object())
    pool = StreamPool(dec, B=3, chunk=4, input_dim=2)
    a = pool.open(context=1)
    b = pool.open()
    c = pool.open(context=0)
    assert dec.resets == [([0], [1]), ([1], [-1]), ([2], [0])]
    pool.close(b)
    pool.open(context=2)                                          # the freed slot, with the new session's graph
    assert dec.resets[-1] == ([1], [2]) and (a, c) == (0, 2)
    plain = _StubDecoder(context=None)
    pool = StreamPool(plain, B=1, chunk=4, input_dim=2)
    with pytest.raises(M3Error):
        pool.open(context=0)
    pool.open()
    assert plain.resets == [([0], None)]


# ------------------------------------------------------------------------------------------------ 7. where the set lives
def test_device_names_are_compared_by_what_they_resolve_to(monkeypatch):
    """CtcBeamSearch(device="cuda") names the current device; the uploaded image's tensor says cuda:<index>."""
    import torch
    from m3asr.decode import _same_device
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    d = torch.device
    assert _same_device(d("cuda"), d("cuda:1")) and _same_device(d("cuda:1"), d("cuda")) and _same_device(d("cuda"), d("cuda"))
    assert not _same_device(d("cuda"), d("cuda:0")) and not _same_device(d("cuda:0"), d("cuda:1"))
    assert _same_device(d("cuda:0"), d("cuda:0")) and _same_device(d("cpu"), d("cpu"))
    assert not _same_device(d("cpu"), d("cuda")) and not _same_device(d("cuda:0"), d("cpu"))
