"""N-gram LM shallow fusion in the device CTC prefix beam search (m3_ctc_beam_lm_*, csrc/ctc_beam.hip) and what is built on it
(CtcBeamSearch / StreamingCtcDecoder / StreamPool with lm=).

Yardstick: the library's fused host routine m3_ctc_prefix_beam_search_lm (pinned on the CPU by tests/test_ctc_lm_host.py
against a pure-Python search and a textbook ARPA scorer) fed with the SAME device top-k pairs: prefixes and their order
identical, CTC score, bonus and lm to 1e-6 (the bound tests/test_ctc_beam_gpu.py and tests/test_ctc_context_gpu.py use).  Where
two device runs are compared (chunking, batching, restarts, LM off) the results must be equal bit for bit.

The order-1 shape of the device == host cases cannot take a back-off step (a unigram LM has state 0 only); "at least one
back-off step" is asserted for the orders that have states to back off from.
"""
import numpy as np
import pytest
import torch

import guarded as G
import lm_ref

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.7, 0.4


def _topk(x, k):
    from m3asr import ops
    return ops.ctc_topk(x.cuda().contiguous(), k)


def _path(x, blank):
    ids = x.argmax(-1).tolist()
    return [t for i, t in enumerate(ids) if t != blank and (i == 0 or t != ids[i - 1])]


def _lm(x, V, order, blank, rng, **kw):
    """a random LM around the greedy path of x (T, V), uploaded"""
    from m3asr.lm import NgramLm
    _, text = lm_ref.arpa_around(_path(x, blank), V, order, rng, blank=blank, **kw)
    return NgramLm.from_arpa(text, None, blank=blank, vocab_size=V).to("cuda")


def _set(graph_phrases, V, blank=0, w=1.5):
    from m3asr.context import ContextGraph, ContextSet
    return ContextSet([ContextGraph(p, V, score=w, blank=blank) for p in graph_phrases], device="cuda")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _lm_search(lp, ix, n_frames, beam, lm, lm_on, cs=None, graph_of=None, blank=0, max_frames=None, chunks=None, alpha=ALPHA,
               beta=BETA, use_eos=True, state=None):
    """ops-level fused search over device top-k pairs (B, T, k); chunks: list of chunk lengths (default: one advance)."""
    from m3asr import ops
    B, T, k = lp.shape
    desc = ops.ctc_beam_desc(B, beam, T if max_frames is None else max_frames, blank, k)
    if state is None:
        state = torch.empty(ops.ctc_beam_lm_state_size(desc), dtype=torch.uint8, device="cuda")
    go = _i32([-1] * B if graph_of is None else graph_of)
    on = _i32(lm_on)
    image = None if cs is None else cs.dev
    lmi = None if lm is None else lm.dev
    ops.ctc_beam_lm_reset(desc, state)
    nf = torch.as_tensor(n_frames, dtype=torch.int64)
    t0 = 0
    for c in (chunks or [T]):
        n_c = (nf - t0).clamp(min=0, max=c).to(torch.int32).cuda()
        ops.ctc_beam_lm_advance(desc, state, image, go, lmi, on, alpha, beta, lp[:, t0:t0 + c].contiguous(),
                                ix[:, t0:t0 + c].contiguous(), n_c)
        t0 += c
    assert t0 == T
    return ops.ctc_beam_lm_nbest(desc, state, image, go, lmi, on, alpha, beta, use_eos)


def _hyps(nb, b):
    toks, hlen, score, bonus, lm, n = (t.cpu() for t in nb)
    return [(tuple(toks[b, i, :int(hlen[b, i])].tolist()), float(score[b, i]), float(bonus[b, i]), float(lm[b, i]))
            for i in range(int(n[b]))]


def _host(lp, ix, b, n, beam, lm, cs=None, graph=-1, blank=0, alpha=ALPHA, beta=BETA, use_eos=True):
    from m3asr import ops
    if n == 0:
        return [((), 0.0, 0.0, float(lm.final[lm.start]) if use_eos else 0.0)]
    got = ops.ctc_prefix_beam_search_lm_host(lp[b, :n].cpu().numpy(), ix[b, :n].cpu().numpy(), beam, blank,
                                             None if cs is None else cs.image, graph, lm.image, alpha, beta, use_eos)
    return [h[:4] for h in got]


def _same_hyps(got, want, tol=1e-6):
    assert [h[0] for h in got] == [h[0] for h in want]
    for i in (1, 2, 3):
        np.testing.assert_allclose([h[i] for h in got], [h[i] for h in want], rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------ 1. device == host
@pytest.mark.parametrize("with_graph", [False, True])
@pytest.mark.parametrize("T,V,beam,blank,order", [(50, 1434, 10, 0, 3), (80, 64, 3, 0, 2), (60, 300, 32, 0, 4), (70, 30, 6, 7, 1)])
def test_device_search_matches_host_lm_routine(T, V, beam, blank, order, with_graph):
    g = torch.Generator().manual_seed(T * 31 + V)
    x = torch.randn(1, T, V, generator=g) * 2.0
    x[:, ::5, blank] += 3.0
    rng = np.random.default_rng(T + V)
    lm = _lm(x[0], V, order, blank, rng)
    path = _path(x[0], blank)
    cs = _set([[path[2:5], path[1:3]]], V, blank) if with_graph else None
    graph = 0 if with_graph else -1
    lp, ix = _topk(x, beam)
    got = _hyps(_lm_search(lp, ix, [T], beam, lm, [1], cs, [graph], blank), 0)
    _same_hyps(got, _host(lp, ix, 0, T, beam, lm, cs, graph, blank))
    assert all(h[3] != 0.0 for h in got), "the case does not exercise the LM"
    if order > 1:
        assert sum(lm.walk(h[0], detail=True)[2] for h in got) > 0, "no back-off step in this case"
    if with_graph:
        assert any(h[2] != 0.0 for h in got), "the case does not exercise the bonus"


# ------------------------------------------------------------------------------------------------ 2. nodes that come back
def test_small_vocab_long_inputs_lm_state_and_sum_return_with_the_node():
    """V = 3..5, T = 300..500, beam 2..8: prefixes leave the beam and re-enter it; their stored (lm_state, lm_sum) must come
    back with the node (a stale or missing pair changes the ranking and the reported lm)."""
    rng = np.random.default_rng(13)
    B = 12
    V = rng.integers(3, 6, B)
    T = rng.integers(300, 501, B)
    beam = rng.integers(2, 9, B)
    for bm in sorted(set(beam.tolist())):
        for Vv in sorted(set(V[beam == bm].tolist())):
            sub = [b for b in range(B) if beam[b] == bm and V[b] == Vv]
            Tm = int(T[sub].max())
            x = torch.from_numpy(rng.normal(0, 1.5, (len(sub), Tm, Vv)).astype(np.float32))
            lm = _lm(x[0], Vv, 4, 0, rng, n_unigrams=Vv, n_higher=12)
            lp, ix = _topk(x, min(bm, Vv))
            nb = _lm_search(lp, ix, [int(T[b]) for b in sub], int(bm), lm, [1] * len(sub), alpha=0.3, beta=0.2)
            for i, b in enumerate(sub):
                _same_hyps(_hyps(nb, i), _host(lp, ix, i, int(T[b]), int(bm), lm, alpha=0.3, beta=0.2))


# ------------------------------------------------------------------------------------------------ 3. resumable, batched
def _batch(seed, B, T, V, beam, order=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * 2.0
    x[:, ::4, 0] += 2.5
    rng = np.random.default_rng(seed)
    lm = _lm(x[0], V, order, 0, rng)
    p0, p1 = _path(x[0], 0), _path(x[1], 0)
    cs = _set([[p0[1:3], p0[4:5]], [p1[0:2], p1[3:6]]], V)
    lp, ix = _topk(x, beam)
    return x, lm, cs, lp, ix


def test_chunked_advances_are_bit_identical():
    B, T, V, beam = 4, 100, 50, 8
    _, lm, cs, lp, ix = _batch(5, B, T, V, beam)
    lens, graph_of, lm_on = [100, 77, 1, 0], [0, 1, -1, 0], [1, 1, 1, 0]
    one = _lm_search(lp, ix, lens, beam, lm, lm_on, cs, graph_of)
    assert float(one[4].abs().max()) > 0 and float(one[3].abs().max()) > 0
    uneven = [1, 7]
    while sum(uneven) < T:
        uneven.append(min(16, T - sum(uneven)))
    for chunks in ([1] * T, [min(7, T - i) for i in range(0, T, 7)], [min(16, T - i) for i in range(0, T, 16)], uneven):
        got = _lm_search(lp, ix, lens, beam, lm, lm_on, cs, graph_of, chunks=chunks)
        for a, b in zip(got, one):
            assert torch.equal(a, b), chunks[:3]


def test_ragged_batch_of_twelve_equals_each_utterance_alone():
    B, T, V, beam = 12, 48, 40, 6
    _, lm, cs, lp, ix = _batch(8, B, T, V, beam)
    rng = np.random.default_rng(8)
    lens = [int(v) for v in rng.integers(0, T + 1, B)]
    lens[0], lens[1] = T, 0
    graph_of = [int(v) for v in rng.integers(-1, 2, B)]
    lm_on = [1] * B
    nb = _lm_search(lp, ix, lens, beam, lm, lm_on, cs, graph_of)
    for b in range(B):
        single = _lm_search(lp[b:b + 1].contiguous(), ix[b:b + 1].contiguous(), [lens[b]], beam, lm, [1], cs, [graph_of[b]],
                            max_frames=T)
        for a, want in zip(nb, single):
            assert G.same_bits(a[b], want[0]), b
        _same_hyps(_hyps(nb, b), _host(lp, ix, b, lens[b], beam, lm, cs, graph_of[b]))


# ------------------------------------------------------------------------------------------------ 4. restart some slots
def test_reset_slots_leaves_the_other_searches_alone():
    from m3asr import ops
    B, T, V, beam = 4, 40, 40, 5
    _, lm, cs, lp, ix = _batch(9, B, T, V, beam)
    desc = ops.ctc_beam_desc(B, beam, T, 0, beam)
    state = torch.empty(ops.ctc_beam_lm_state_size(desc), dtype=torch.uint8, device="cuda")
    go, on = _i32([0, 1, -1, 0]), _i32([1, 1, 1, 0])
    half = _i32([20] * B)
    args = (cs.dev, go, lm.dev, on, ALPHA, BETA)
    ops.ctc_beam_lm_reset(desc, state)
    ops.ctc_beam_lm_advance(desc, state, *args, lp[:, :20].contiguous(), ix[:, :20].contiguous(), half)
    before = ops.ctc_beam_lm_nbest(desc, state, *args, True)
    ops.ctc_beam_lm_reset(desc, state, _i32([1, 3, 7, -2]))        # entries outside [0, B) are skipped
    after = ops.ctc_beam_lm_nbest(desc, state, *args, True)
    for a, b in zip(before, after):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert after[5].cpu().tolist()[1::2] == [1, 1] and after[1][1, 0].item() == 0 and after[1][3, 0].item() == 0
    # the restarted slots run the second half as fresh searches; the others go on as if nothing had happened
    ops.ctc_beam_lm_advance(desc, state, *args, lp[:, 20:].contiguous(), ix[:, 20:].contiguous(), half)
    got = ops.ctc_beam_lm_nbest(desc, state, *args, True)
    whole = _lm_search(lp, ix, [40] * B, beam, lm, [1, 1, 1, 0], cs, [0, 1, -1, 0])
    tail = _lm_search(lp[:, 20:].contiguous(), ix[:, 20:].contiguous(), [20] * B, beam, lm, [1, 1, 1, 0], cs, [0, 1, -1, 0],
                      max_frames=T)
    for a, w, t in zip(got, whole, tail):
        assert torch.equal(a[0], w[0]) and torch.equal(a[2], w[2]) and torch.equal(a[1], t[1]) and torch.equal(a[3], t[3])


# ------------------------------------------------------------------------------------------------ 5. LM off == ctx search
def test_lm_off_or_zero_weights_are_the_ctx_search_bit_for_bit():
    from m3asr import ops
    B, T, V, beam = 4, 64, 40, 6
    _, lm, cs, lp, ix = _batch(6, B, T, V, beam)
    lens, graph_of = [64, 64, 50, 33], [-1, 0, 1, 0]
    desc = ops.ctc_beam_desc(B, beam, T, 0, beam)
    state = torch.empty(ops.ctc_beam_ctx_state_size(desc), dtype=torch.uint8, device="cuda")
    ops.ctc_beam_ctx_reset(desc, state)
    ops.ctc_beam_ctx_advance(desc, state, cs.dev, _i32(graph_of), lp, ix, _i32(lens))
    c_toks, c_hlen, c_score, c_bonus, c_n = ops.ctc_beam_ctx_nbest(desc, state, cs.dev, _i32(graph_of))
    # a mixed batch: rows 0 and 2 run without the LM, rows 1 and 3 with it
    toks, hlen, score, bonus, hlm, n = _lm_search(lp, ix, lens, beam, lm, [0, 1, 0, 1], cs, graph_of)
    for b in (0, 2):
        assert torch.equal(toks[b], c_toks[b]) and torch.equal(hlen[b], c_hlen[b]) and torch.equal(n[b], c_n[b])
        assert G.same_bits(score[b], c_score[b]) and G.same_bits(bonus[b], c_bonus[b]) and bool((hlm[b] == 0).all())
    assert not torch.equal(toks[1], c_toks[1]) and float(hlm[1].abs().max()) > 0 and float(hlm[3].abs().max()) > 0
    # the LM on, but without weight and without </s>: the same ranking, and hyp_lm still reports the LM score
    zero = _lm_search(lp, ix, lens, beam, lm, [1] * B, cs, graph_of, alpha=0.0, beta=0.0, use_eos=False)
    assert torch.equal(zero[0], c_toks) and torch.equal(zero[1], c_hlen) and torch.equal(zero[5], c_n)
    assert G.same_bits(zero[2], c_score) and G.same_bits(zero[3], c_bonus) and float(zero[4].abs().max()) > 0
    # no LM image at all, and a header that fails its check: "LM off"
    none = _lm_search(lp, ix, lens, beam, None, [1] * B, cs, graph_of)
    assert torch.equal(none[0], c_toks) and G.same_bits(none[2], c_score) and bool((none[4] == 0).all())

    import types
    broken = types.SimpleNamespace(dev=lm.dev.clone())
    broken.dev[1] = 99                                            # the version word
    bad = _lm_search(lp, ix, lens, beam, broken, [1] * B, cs, graph_of)
    assert torch.equal(bad[0], c_toks) and G.same_bits(bad[2], c_score) and bool((bad[4] == 0).all())


# ------------------------------------------------------------------------------------------------ 6. guarded operands
def test_guarded_and_strided_operands():
    """Every operand inside guard memory (the ABI has no strides for them, so the guards are flat): inputs surrounded by NaN
    or by integers that are harmless as indices, both images inside larger word buffers, the outputs and the state by a bit
    pattern that must survive."""
    from m3asr import ops
    B, T, V, beam = 3, 30, 40, 5
    _, lm, cs, lp, ix = _batch(11, B, T, V, beam)
    lens, graph_of, lm_on = [30, 17, 0], [0, -1, 1], [1, 1, 0]
    want = _lm_search(lp, ix, lens, beam, lm, lm_on, cs, graph_of)
    desc = ops.ctc_beam_desc(B, beam, T, 0, beam)
    g_state = G.flat_out((ops.ctc_beam_lm_state_size(desc),), torch.uint8)
    g_lp = G.flat_in(lp.cpu(), int_guard=None)
    g_ix = G.flat_in(ix.cpu(), int_guard=V + 5)                   # a consumed guard id is a token the LM does not know
    g_nf = G.flat_in(torch.tensor(lens, dtype=torch.int32), int_guard=0)
    g_go = G.flat_in(torch.tensor(graph_of, dtype=torch.int32), int_guard=-1)
    g_on = G.flat_in(torch.tensor(lm_on, dtype=torch.int32), int_guard=0)
    g_lm = G.flat_in(lm.dev.cpu(), int_guard=-1)
    g_cs = G.flat_in(cs.dev.cpu(), int_guard=-1)
    ops.ctc_beam_lm_reset(desc, g_state.view)
    ops.ctc_beam_lm_advance(desc, g_state.view, g_cs.view, g_go.view, g_lm.view, g_on.view, ALPHA, BETA, g_lp.view, g_ix.view,
                            g_nf.view)
    g_state.check("ctc beam lm state")
    lib, C = ops._lib.load(), ops.C
    outs = [G.flat_out((B, beam, T), torch.int32), G.flat_out((B, beam), torch.int32), G.flat_out((B, beam)), G.flat_out((B, beam)),
            G.flat_out((B, beam)), G.flat_out((B,), torch.int32)]
    p = lambda t: C.c_void_p(t.data_ptr())
    ops.check(lib.m3_ctc_beam_lm_nbest(C.byref(desc), p(g_state.view), g_state.view.numel(), p(g_cs.view), g_cs.view.numel() * 4,
                                       p(g_go.view), p(g_lm.view), g_lm.view.numel() * 4, p(g_on.view), ALPHA, BETA, 1,
                                       *[p(o.view) for o in outs], ops._stream()), "m3_ctc_beam_lm_nbest")
    for o, w, name in zip(outs, want, ("hyp_tokens", "hyp_len", "hyp_score", "hyp_bonus", "hyp_lm", "n_hyps")):
        o.check(name)
        assert G.same_bits(o.view, w), name
    g_state.check("ctc beam lm state after nbest")


# ------------------------------------------------------------------------------------------------ 7. overflow
def test_overflow_is_sticky_and_nothing_is_written_outside_the_state():
    from m3asr import ops
    B, beam, F, V = 3, 4, 10, 20
    x = torch.randn(B, 8, V, generator=torch.Generator().manual_seed(7))
    lm = _lm(x[0], V, 3, 0, np.random.default_rng(7))
    cs = _set([[[1, 2], [3]], [[4]]], V)
    desc = ops.ctc_beam_desc(B, beam, F, 0)
    n = ops.ctc_beam_lm_state_size(desc)
    assert n > ops.ctc_beam_ctx_state_size(desc)
    gs = G.flat_out((n,), torch.uint8)
    state = gs.view
    args = (cs.dev, _i32([0, 1, -1]), lm.dev, _i32([1, 1, 1]), ALPHA, BETA)
    ops.ctc_beam_lm_reset(desc, state)
    lp, ix = ops.ctc_topk(x.cuda(), beam)
    ops.ctc_beam_lm_advance(desc, state, *args, lp, ix, _i32([8, 8, 2]))
    ops.ctc_beam_lm_advance(desc, state, *args, lp, ix, _i32([3, 2, 8]))            # 11 > 10 for b = 0
    nh = ops.ctc_beam_lm_nbest(desc, state, *args)[5].cpu().tolist()
    assert nh[0] == -1 and nh[1] > 0 and nh[2] > 0
    ops.ctc_beam_lm_advance(desc, state, *args, lp, ix, _i32([1, 0, 0]))            # sticky
    ops.ctc_beam_lm_reset(desc, state, _i32([1]))                                   # another slot's restart changes nothing
    assert ops.ctc_beam_lm_nbest(desc, state, *args)[5].cpu().tolist()[0] == -1
    gs.check("ctc beam lm state")
    # exactly max_frames frames: the last survivors take the last nodes of the pool, none past it
    ops.ctc_beam_lm_reset(desc, state)
    ops.ctc_beam_lm_advance(desc, state, *args, lp, ix, _i32([8, 8, 8]))
    ops.ctc_beam_lm_advance(desc, state, *args, lp[:, :2].contiguous(), ix[:, :2].contiguous(), _i32([2, 2, 2]))
    nb = ops.ctc_beam_lm_nbest(desc, state, *args)
    assert min(nb[5].cpu().tolist()) > 0
    gs.check("ctc beam lm state, pool full")
    full = torch.cat([lp, lp[:, :2]], 1), torch.cat([ix, ix[:, :2]], 1)
    _same_hyps(_hyps(nb, 0), _host(full[0], full[1], 0, 10, beam, lm, cs, 0))


# ------------------------------------------------------------------------------------------------ 8. classes
def test_beam_search_class_flips_a_tie_with_the_lm_weight():
    from m3asr.decode import CtcBeamSearch
    from m3asr.lm import NgramLm
    V = 6
    p = torch.full((6, V), 1e-7)
    for t, tok in enumerate([1, 0, 2, 0, None, 0]):
        if tok is None:                                           # 4 before 3, 0.04 nat apart; the LM prefers 3 by 2 nat
            p[t, 4], p[t, 3] = 0.51, 0.49 - 4e-7
        else:
            p[t, tok] = 1.0 - 5e-7
    logits = p.log()[None].cuda()
    text = ("\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-1.0\t1\t-0.2\n-1.0\t2\t-0.2\n-1.0\t3\n-1.0\t4\n-1.0\t5\n\n"
            "\\2-grams:\n-0.2\t1 2\n-0.1\t2 3\n-1.0\t2 4\n\n\\end\\\n")
    lm = NgramLm.from_arpa(text, None, vocab_size=V).to("cuda")

    def run(weight):
        s = CtcBeamSearch(1, 6, 6, lm=lm, lm_weight=weight, lm_eos=False)
        s.advance(logits, torch.tensor([6]))
        assert [h[:2] for h in s.nbest(detail=True)[0]] == s.nbest()[0]     # without detail: the plain search's tuples
        return s.nbest(detail=True)[0]

    off, on = run(0.0), run(1.0)
    assert off[0][0] == (1, 2, 4) and off[1][0] == (1, 2, 3) and on[0][0] == (1, 2, 3) and on[1][0] == (1, 2, 4)
    assert on[0][3] == pytest.approx(lm.score((1, 2, 3)), abs=1e-5) and on[0][1] == pytest.approx(off[1][1], abs=1e-6)
    with pytest.raises(ops_error()):
        CtcBeamSearch(1, 6, 6, lm=NgramLm.from_arpa(text, None, vocab_size=V))     # not uploaded


def _engine(seed):
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=16,
                        num_decoding_left_chunks=2)
    return cfg, Engine.from_state_dict(cfg, make_weights(cfg, seed=seed), packed_rows=False)


def test_streaming_decoder_with_lm_equals_batched_search():
    from m3asr.config import subsampled_len
    from m3asr.decode import CtcBeamSearch, StreamingCtcDecoder
    cfg, eng = _engine(41)
    lengths = [206, 150, 64]
    B, c, beam = len(lengths), 16, 5
    feat = torch.rand(B, max(lengths), cfg.input_dim, generator=torch.Generator().manual_seed(10))
    fl = torch.tensor(lengths, dtype=torch.int32)
    T = feat.shape[1]
    Tp = subsampled_len(T)
    total = torch.tensor([subsampled_len(v) for v in lengths])
    st = eng.streaming(B, Tp)
    full = st.decode(feat, fl).cpu()                              # the logits the LM is built around
    V = full.shape[-1]
    lm = _lm(full[0, :int(total[0])], V, 3, 0, np.random.default_rng(3))
    kw = dict(lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    dec = StreamingCtcDecoder(st, beam, **kw)
    dec.reset(lm_on=[True, True, False])
    n_chunks = -(-Tp // c)
    padded = torch.zeros(B, max(T, 4 * c * n_chunks + 3), feat.shape[2])
    padded[:, :T] = feat
    seen = []
    for n in range(n_chunks):
        left = (fl.long() - 4 * c * n).clamp(min=0, max=st.window)
        left = torch.where(left >= 7, left, torch.zeros_like(left))
        lg = dec.step(padded[:, 4 * c * n: 4 * c * n + st.window], left, (total - n * c).clamp(min=0, max=c))   # graph replay
        eng.stream.synchronize()
        seen.append(lg.clone())
    got = dec.finish(detail=True)
    s = CtcBeamSearch(B, beam, Tp, **kw)
    s.reset(lm_on=[True, True, False])
    s.advance(torch.cat(seen, 1).contiguous(), total)
    assert got == s.nbest(detail=True)
    assert all(h[3] != 0.0 for h in got[0] + got[1]) and all(h[3] == 0.0 for h in got[2])
    plain = CtcBeamSearch(B, beam, Tp)
    plain.advance(torch.cat(seen, 1).contiguous(), total)
    assert [h[:2] for h in got[2]] == plain.nbest()[2] and [h[0] for h in got[0]] != [h[0] for h in plain.nbest()[0]]


def test_stream_pool_with_one_lm_slot_and_one_plain_slot():
    from m3asr.config import subsampled_len
    from m3asr.decode import StreamingCtcDecoder
    from m3asr.serve import StreamPool
    cfg, eng = _engine(46)
    utt = torch.rand(150, cfg.input_dim, generator=torch.Generator().manual_seed(13))
    Tp = subsampled_len(150)
    logits = eng.streaming(2, Tp).decode(utt[None].repeat(2, 1, 1), torch.tensor([150, 150], dtype=torch.int32)).cpu()
    lm = _lm(logits[0, :Tp], logits.shape[-1], 3, 0, np.random.default_rng(4))

    def run(dec, flags):
        pool = StreamPool(dec)
        sids = [pool.open(lm=f) if f is not None else pool.open() for f in flags]
        for sid in sids:
            pool.push(sid, utt)
            pool.end(sid)
        for _ in range(40):
            if not any(pool.pending(sid) for sid in sids):
                break
            pool.step()
        return [pool.close(sid) for sid in sids]

    fused = StreamingCtcDecoder(eng.streaming(2, Tp, independent=True), beam=5, lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    with_lm, without = run(fused, [True, False])
    both = run(fused, [None, True])                               # the same slots again: the flags are per session
    plain = run(StreamingCtcDecoder(eng.streaming(2, Tp, independent=True), beam=5), [None, None])
    assert without == plain[1] and plain[0] == plain[1]
    assert with_lm == both[0] == both[1] and [h[0] for h in with_lm] != [h[0] for h in without]
    with pytest.raises(ops_error()):
        StreamPool(StreamingCtcDecoder(eng.streaming(2, Tp, independent=True), beam=5)).open(lm=True)


def ops_error():
    from m3asr._lib import M3Error
    return M3Error
