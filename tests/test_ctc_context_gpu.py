"""Hotword biasing of the device CTC prefix beam search (m3_ctc_beam_ctx_*, csrc/ctc_beam.hip) and what is built on it
(CtcBeamSearch / StreamingCtcDecoder with context=).

Yardstick: the library's biased host routine m3_ctc_prefix_beam_search_ctx (pinned on the CPU by
tests/test_ctc_context_host.py against a pure-Python search and a brute-force phrase count) fed with the SAME device top-k
pairs: prefixes and their order identical, CTC score and bonus to 1e-6 (the bound tests/test_ctc_beam_gpu.py uses).  Where two
device runs are compared (chunking, batching, restarts) the results must be equal bit for bit.
"""
import numpy as np
import pytest
import torch

import guarded as G

pytestmark = pytest.mark.gpu

W = 3.0


def _topk(x, k):
    from m3asr import ops
    return ops.ctc_topk(x.cuda().contiguous(), k)


def _ctx_search(lp, ix, n_frames, beam, cs, graph_of, blank=0, max_frames=None, chunks=None):
    """ops-level biased search over device top-k pairs (B, T, k); chunks: list of chunk lengths (default: one advance)."""
    from m3asr import ops
    B, T, k = lp.shape
    desc = ops.ctc_beam_desc(B, beam, T if max_frames is None else max_frames, blank, k)
    state = torch.empty(ops.ctc_beam_ctx_state_size(desc), dtype=torch.uint8, device="cuda")
    go = torch.tensor(graph_of, dtype=torch.int32).cuda()
    ops.ctc_beam_ctx_reset(desc, state)
    nf = torch.as_tensor(n_frames, dtype=torch.int64)
    t0 = 0
    for c in (chunks or [T]):
        n_c = (nf - t0).clamp(min=0, max=c).to(torch.int32).cuda()
        ops.ctc_beam_ctx_advance(desc, state, cs.dev, go, lp[:, t0:t0 + c].contiguous(), ix[:, t0:t0 + c].contiguous(), n_c)
        t0 += c
    assert t0 == T
    return ops.ctc_beam_ctx_nbest(desc, state, cs.dev, go)


def _hyps(nb, b):
    toks, hlen, score, bonus, n = (t.cpu() for t in nb)
    return [(tuple(toks[b, i, :int(hlen[b, i])].tolist()), float(score[b, i]), float(bonus[b, i])) for i in range(int(n[b]))]


def _host(lp, ix, b, n, beam, cs, graph, blank=0):
    from m3asr import ops
    if n == 0:
        return [((), 0.0, 0.0)]
    got = ops.ctc_prefix_beam_search_ctx_host(lp[b, :n].cpu().numpy(), ix[b, :n].cpu().numpy(), beam, blank, cs.image, graph)
    return [h[:3] for h in got]


def _same_hyps(got, want, tol=1e-6):
    assert [h[0] for h in got] == [h[0] for h in want]
    np.testing.assert_allclose([h[1] for h in got], [h[1] for h in want], rtol=tol, atol=tol)
    np.testing.assert_allclose([h[2] for h in got], [h[2] for h in want], rtol=tol, atol=tol)


def _phrases(x, V, blank, n, rng, lo=2, hi=6):
    """n phrases of lo..hi tokens: half cut from the greedy path of x (T, V), half noise"""
    ids = x.argmax(-1).tolist()
    path = [t for i, t in enumerate(ids) if t != blank and (i == 0 or t != ids[i - 1])]
    out = set()
    for _ in range(1000):
        if len(out) >= n // 2:
            break
        m = int(rng.integers(lo, hi + 1))
        if len(path) > m:
            i = int(rng.integers(0, len(path) - m))
            out.add(tuple(path[i:i + m]))
    toks = [t for t in range(V) if t != blank]
    while len(out) < n:
        out.add(tuple(int(toks[i]) for i in rng.integers(0, len(toks), int(rng.integers(lo, hi + 1)))))
    return [list(p) for p in sorted(out)]


def _set(graph_phrases, V, blank=0, w=W):
    from m3asr.context import ContextGraph, ContextSet
    return ContextSet([ContextGraph(p, V, score=w, blank=blank) for p in graph_phrases], device="cuda")


# ------------------------------------------------------------------------------------------------ 1. device == host
@pytest.mark.parametrize("T,V,beam,blank,n_phrases", [(50, 1434, 10, 0, 20), (80, 64, 3, 0, 8), (60, 300, 32, 0, 12),
                                                      (70, 30, 6, 7, 6)])
def test_device_search_matches_host_ctx_routine(T, V, beam, blank, n_phrases):
    g = torch.Generator().manual_seed(T * 31 + V)
    x = torch.randn(1, T, V, generator=g) * 2.0
    x[:, ::5, blank] += 3.0
    rng = np.random.default_rng(T + V)
    cs = _set([[[t] for t in range(V) if t != blank][:3], _phrases(x[0], V, blank, n_phrases, rng)], V, blank)
    lp, ix = _topk(x, beam)
    got = _hyps(_ctx_search(lp, ix, [T], beam, cs, [1], blank), 0)
    _same_hyps(got, _host(lp, ix, 0, T, beam, cs, 1, blank))
    assert any(h[2] != 0.0 for h in got), "the case does not exercise the bonus"


# ------------------------------------------------------------------------------------------------ 2. nodes that come back
def test_small_vocab_long_inputs_state_and_bonus_return_with_the_node():
    """V = 3..5, T = 300..500, beam 2..8: prefixes leave the beam and re-enter it; their stored state and bonus must come
    back with the node (a stale or missing pair changes the ranking and the reported bonus)."""
    rng = np.random.default_rng(12)
    B = 12
    V = rng.integers(3, 6, B)
    T = rng.integers(300, 501, B)
    beam = rng.integers(2, 9, B)
    for bm in sorted(set(beam.tolist())):
        for Vv in sorted(set(V[beam == bm].tolist())):
            sub = [b for b in range(B) if beam[b] == bm and V[b] == Vv]
            Tm = int(T[sub].max())
            phrases = _phrases(torch.zeros(1, Vv), Vv, 0, 4, rng, lo=1, hi=3)
            cs = _set([phrases], Vv, w=1.25)
            x = torch.from_numpy(rng.normal(0, 1.5, (len(sub), Tm, Vv)).astype(np.float32))
            lp, ix = _topk(x, min(bm, Vv))
            nb = _ctx_search(lp, ix, [int(T[b]) for b in sub], int(bm), cs, [0] * len(sub))
            for i, b in enumerate(sub):
                _same_hyps(_hyps(nb, i), _host(lp, ix, i, int(T[b]), int(bm), cs, 0))


# ------------------------------------------------------------------------------------------------ 3. resumable
def _batch(seed, B, T, V, beam):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * 2.0
    x[:, ::4, 0] += 2.5
    rng = np.random.default_rng(seed)
    cs = _set([_phrases(x[0], V, 0, 8, rng, 1, 4), _phrases(x[1], V, 0, 8, rng, 1, 4)], V)
    lp, ix = _topk(x, beam)
    return x, cs, lp, ix


def test_chunked_advances_are_bit_identical():
    B, T, V, beam = 4, 100, 50, 8
    _, cs, lp, ix = _batch(5, B, T, V, beam)
    lens, graph_of = [100, 77, 1, 0], [0, 1, -1, 0]
    one = _ctx_search(lp, ix, lens, beam, cs, graph_of)
    assert float(one[3].abs().max()) > 0
    uneven = [1, 7]
    while sum(uneven) < T:
        uneven.append(min(16, T - sum(uneven)))
    for chunks in ([min(16, T - i) for i in range(0, T, 16)], uneven):
        got = _ctx_search(lp, ix, lens, beam, cs, graph_of, chunks=chunks)
        for a, b in zip(got, one):
            assert torch.equal(a, b), chunks


# ------------------------------------------------------------------------------------------------ 4. mixed batch
def test_mixed_batch_unbiased_row_and_single_runs():
    from m3asr import ops
    B, T, V, beam = 4, 64, 40, 6
    _, cs, lp, ix = _batch(6, B, T, V, beam)
    lens, graph_of = [64, 64, 50, 33], [-1, 0, 1, 0]
    toks, hlen, score, bonus, n = _ctx_search(lp, ix, lens, beam, cs, graph_of)
    # row 0: the unbiased search, exactly
    desc = ops.ctc_beam_desc(1, beam, T, 0, beam)
    state = torch.empty(ops.ctc_beam_state_size(desc), dtype=torch.uint8, device="cuda")
    ops.ctc_beam_reset(desc, state)
    ops.ctc_beam_advance(desc, state, lp[:1].contiguous(), ix[:1].contiguous(), torch.tensor([lens[0]], dtype=torch.int32).cuda())
    u_toks, u_hlen, u_score, u_n = ops.ctc_beam_nbest(desc, state)
    assert torch.equal(toks[0], u_toks[0]) and torch.equal(hlen[0], u_hlen[0]) and torch.equal(n[:1], u_n)
    assert G.same_bits(score[0], u_score[0]) and bool((bonus[0] == 0).all())
    # an out-of-range graph id is "unbiased" too
    far = _ctx_search(lp[:1].contiguous(), ix[:1].contiguous(), lens[:1], beam, cs, [len(cs)])
    assert torch.equal(far[0][0], u_toks[0]) and G.same_bits(far[2][0], u_score[0]) and bool((far[3] == 0).all())
    # rows 1..3: single-utterance runs
    for b in (1, 2, 3):
        single = _ctx_search(lp[b:b + 1].contiguous(), ix[b:b + 1].contiguous(), [lens[b]], beam, cs, [graph_of[b]], max_frames=T)
        for a, want in zip((toks, hlen, score, bonus, n), single):
            assert G.same_bits(a[b], want[0]), b
    assert float(bonus[1:].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5. restart one slot
def test_restart_one_slot_with_another_graph():
    from m3asr._lib import M3Error
    from m3asr.decode import CtcBeamSearch
    B, T, V, beam = 4, 60, 40, 5
    x, cs, _, _ = _batch(7, B, T, V, beam)
    y = torch.randn(1, 40, V, generator=torch.Generator().manual_seed(70)) * 2.0
    x, y = x.cuda(), y.cuda()
    s = CtcBeamSearch(B, beam, T, context=cs)
    s.set_context([0, 1, 2, 3], [0, 1, 0, -1])
    s.reset()
    s.advance(x[:, :20].contiguous(), torch.full((B,), 20))
    with pytest.raises(M3Error):
        s.set_context([2], [1])                                   # slot 2 has consumed frames
    s.reset(slots=[2], graph_ids=[1])
    second = x[:, 20:].clone()
    second[2] = y[0]
    s.advance(second, torch.full((B,), 40))
    got = s.nbest(detail=True)
    for b, (frames, graph) in enumerate([(x[0:1], 0), (x[1:2], 1), (y, 1), (x[3:4], -1)]):
        fresh = CtcBeamSearch(1, beam, T, context=cs)
        fresh.reset(graph_ids=[graph])
        fresh.advance(frames.contiguous(), torch.tensor([frames.shape[1]]))
        assert got[b] == fresh.nbest(detail=True)[0], b
    assert [h[:2] for h in got[1]] == s.nbest()[1]                # without detail: the tuple shape of the unbiased search


# ------------------------------------------------------------------------------------------------ 6. by hand
def test_hand_built_case_flips_only_with_the_matching_phrase():
    from m3asr.decode import CtcBeamSearch
    V, w = 6, W
    # every frame but one is all but certain, so that what a beam of 6 prunes changes no score by 1e-6; frame 4 decides
    p = torch.full((6, V), 1e-7)
    for t, tok in enumerate([1, 0, 2, 0, None, 0]):
        if tok is None:                                           # 4 before 3, log(0.55 / 0.45) = 0.2 < w apart
            p[t, 4], p[t, 3] = 0.55, 0.45 - 4e-7
        else:
            p[t, tok] = 1.0 - 5e-7
    logits = p.log()[None].cuda()

    def run(phrases):
        cs = _set([phrases], V, w=w)
        s = CtcBeamSearch(1, 6, 6, context=cs)
        s.reset(graph_ids=[0])
        s.advance(logits, torch.tensor([6]))
        return s.nbest(detail=True)[0]

    plain = CtcBeamSearch(1, 6, 6)
    plain.advance(logits, torch.tensor([6]))
    u = plain.nbest()[0]
    assert u[0][0] == (1, 2, 4) and u[1][0] == (1, 2, 3) and 0 < u[0][1] - u[1][1] < w
    ctc = dict(u)
    hit = run([[1, 2, 3]])
    assert hit[0][0] == (1, 2, 3) and hit[1][0] == (1, 2, 4)                       # the order flips
    assert hit[0][2] == pytest.approx(3 * w, abs=1e-6) and hit[1][2] == 0.0
    for prefix, score, _ in hit[:2]:
        assert score == pytest.approx(ctc[prefix], abs=1e-6)     # the CTC scores are unchanged
    miss = run([[1, 2, 5]])
    assert miss[0][0] == (1, 2, 4) and miss[0][2] == 0.0
    assert miss[0][1] == pytest.approx(ctc[(1, 2, 4)], abs=1e-6)


# ------------------------------------------------------------------------------------------------ 7. on the streaming engine
def test_streaming_decoder_with_context_equals_batched_search():
    from m3asr.config import EncoderConfig, subsampled_len
    from m3asr.decode import CtcBeamSearch, StreamingCtcDecoder
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=16,
                        num_decoding_left_chunks=2)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=41), packed_rows=False)
    lengths = [206, 150, 64]
    B, c, beam = len(lengths), 16, 5
    g = torch.Generator().manual_seed(10)
    feat = torch.rand(B, max(lengths), cfg.input_dim, generator=g)
    fl = torch.tensor(lengths, dtype=torch.int32)
    T = feat.shape[1]
    Tp = subsampled_len(T)
    total = torch.tensor([subsampled_len(v) for v in lengths])
    st = eng.streaming(B, Tp)
    full = st.decode(feat, fl).cpu()                              # the logits the phrases are cut from
    rng = np.random.default_rng(3)
    V = full.shape[-1]
    cs = _set([_phrases(full[0, :int(total[0])], V, 0, 6, rng, 1, 3), _phrases(full[1, :int(total[1])], V, 0, 6, rng, 1, 3)], V)
    graph_ids = [0, 1, -1]
    dec = StreamingCtcDecoder(st, beam, context=cs)
    dec.reset(graph_ids=graph_ids)
    n_chunks = -(-Tp // c)
    padded = torch.zeros(B, max(T, 4 * c * n_chunks + 3), feat.shape[2])
    padded[:, :T] = feat
    seen = []
    for n in range(n_chunks):
        left = (fl.long() - 4 * c * n).clamp(min=0, max=st.window)
        left = torch.where(left >= 7, left, torch.zeros_like(left))
        lg = dec.step(padded[:, 4 * c * n: 4 * c * n + st.window], left, (total - n * c).clamp(min=0, max=c))
        eng.stream.synchronize()
        seen.append(lg.clone())
    got = dec.finish(detail=True)
    s = CtcBeamSearch(B, beam, Tp, context=cs)
    s.reset(graph_ids=graph_ids)
    s.advance(torch.cat(seen, 1).contiguous(), total)
    assert got == s.nbest(detail=True)
    assert any(h[2] != 0.0 for h in got[0] + got[1]) and all(h[2] == 0.0 for h in got[2])


# ------------------------------------------------------------------------------------------------ 8. overflow
def test_overflow_is_sticky_and_nothing_is_written_outside_the_state():
    from m3asr import ops
    B, beam, F, V = 3, 4, 10, 20
    cs = _set([[[1, 2], [3]], [[4]]], V)
    desc = ops.ctc_beam_desc(B, beam, F, 0)
    n = ops.ctc_beam_ctx_state_size(desc)
    assert n > ops.ctc_beam_state_size(desc)
    gs = G.flat_out((n,), torch.uint8)
    state = gs.view
    go = torch.tensor([0, 1, -1], dtype=torch.int32).cuda()
    ops.ctc_beam_ctx_reset(desc, state)
    x = torch.randn(B, 8, V, generator=torch.Generator().manual_seed(7)).cuda()
    lp, ix = ops.ctc_topk(x, beam)
    nf = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    ops.ctc_beam_ctx_advance(desc, state, cs.dev, go, lp, ix, nf([8, 8, 2]))
    ops.ctc_beam_ctx_advance(desc, state, cs.dev, go, lp, ix, nf([3, 2, 8]))        # 11 > 10 for b = 0
    nh = ops.ctc_beam_ctx_nbest(desc, state, cs.dev, go)[4].cpu().tolist()
    assert nh[0] == -1 and nh[1] > 0 and nh[2] > 0
    ops.ctc_beam_ctx_advance(desc, state, cs.dev, go, lp, ix, nf([1, 0, 0]))        # sticky
    ops.ctc_beam_ctx_reset(desc, state, torch.tensor([1], dtype=torch.int32).cuda())  # another slot's restart changes nothing
    assert ops.ctc_beam_ctx_nbest(desc, state, cs.dev, go)[4].cpu().tolist()[0] == -1
    gs.check("ctc beam ctx state")
    # exactly max_frames frames: the last survivors take the last nodes of the pool, none past it
    ops.ctc_beam_ctx_reset(desc, state)
    ops.ctc_beam_ctx_advance(desc, state, cs.dev, go, lp, ix, nf([8, 8, 8]))
    ops.ctc_beam_ctx_advance(desc, state, cs.dev, go, lp[:, :2].contiguous(), ix[:, :2].contiguous(), nf([2, 2, 2]))
    assert min(ops.ctc_beam_ctx_nbest(desc, state, cs.dev, go)[4].cpu().tolist()) > 0
    gs.check("ctc beam ctx state, pool full")
