"""Batched, resumable CTC prefix beam search on the device (m3_ctc_beam_*, csrc/ctc_beam.hip), the streaming greedy search
(m3_ctc_greedy_stream_*) and the decoders built on them (CtcBeamSearch, CtcDecoder.batch_prefix_beam_search, chunked
CtcDecoder, StreamingCtcDecoder).

Yardsticks: the reference's n-best lists (tests/golden/ctc_decode.npz, 1e-4 as in tests/test_ctc_decode.py) and the library's
host routine m3_ctc_prefix_beam_search (itself pinned to that fixture) fed with the SAME top-k pairs: prefixes and their order
identical, scores to 1e-6.  Chunked advances must give the bits of one advance.
"""
import os

import numpy as np
import pytest
import torch

from oracle import ctc_decode as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_decode.npz")


def _same_hyps(got, want, tol=1e-6):
    assert [p for p, _ in got] == [p for p, _ in want]
    np.testing.assert_allclose([s for _, s in got], [s for _, s in want], rtol=tol, atol=tol)


def _device_search(lp, ix, n_frames, beam, blank=0, max_frames=None, chunks=None):
    """ops-level search over device top-k pairs (B, T, k); chunks: list of chunk lengths (default: one advance)."""
    from m3asr import ops
    B, T, k = lp.shape
    desc = ops.ctc_beam_desc(B, beam, T if max_frames is None else max_frames, blank, k)
    state = torch.empty(ops.ctc_beam_state_size(desc), dtype=torch.uint8, device="cuda")
    ops.ctc_beam_reset(desc, state)
    nf = torch.as_tensor(n_frames, dtype=torch.int64)
    t0 = 0
    for c in (chunks or [T]):
        n_c = (nf - t0).clamp(min=0, max=c).to(torch.int32).cuda()
        ops.ctc_beam_advance(desc, state, lp[:, t0:t0 + c].contiguous(), ix[:, t0:t0 + c].contiguous(), n_c)
        t0 += c
    assert t0 == T
    return ops.ctc_beam_nbest(desc, state)


def _hyps(nb, b):
    toks, hlen, score, n = (t.cpu() for t in nb)
    return [(tuple(toks[b, i, :int(hlen[b, i])].tolist()), float(score[b, i])) for i in range(int(n[b]))]


def _host(lp, ix, b, n, beam, blank=0):
    from m3asr import ops
    return ops.ctc_prefix_beam_search_host(lp[b, :n].cpu().numpy(), ix[b, :n].cpu().numpy(), beam, blank)


def _topk(x, k):
    from m3asr import ops
    return ops.ctc_topk(x.cuda().contiguous(), k)


# ------------------------------------------------------------------------------------------------ 1. reference fixture
def test_device_search_matches_reference_fixture():
    from m3asr.decode import CtcBeamSearch
    z = np.load(GOLDEN, allow_pickle=False)
    for name in z["beam_cases"]:
        name = str(name)
        blank, beam = (int(v) for v in z[name + "_meta"])
        logits = torch.from_numpy(z[name + "_logits"]).cuda()[None]
        s = CtcBeamSearch(1, beam, logits.shape[1], blank)
        s.advance(logits, torch.tensor([logits.shape[1]]))
        n = int(z[name + "_n"][0])
        toks, ln, sc = z[name + "_hyp_tokens"], z[name + "_hyp_len"], z[name + "_hyp_score"]
        want = [(tuple(int(v) for v in toks[i, :ln[i]]), float(sc[i])) for i in range(n)]
        _same_hyps(s.nbest()[0], want, 1e-4)


# ------------------------------------------------------------------------------------------------ 2. host routine, random
@pytest.mark.parametrize("T,V,beam,blank", [(50, 1434, 10, 0), (17, 9, 9, 0), (80, 64, 3, 0), (60, 40, 1, 0), (60, 300, 32, 0),
                                            (70, 30, 6, 7)])
def test_device_search_matches_host_routine(T, V, beam, blank):
    g = torch.Generator().manual_seed(T * 31 + V)
    x = torch.randn(1, T, V, generator=g) * 2.0
    x[:, ::5, blank] += 3.0                      # blanks win often enough for merges and repeats
    lp, ix = _topk(x, beam)
    got = _hyps(_device_search(lp, ix, [T], beam, blank), 0)
    _same_hyps(got, _host(lp, ix, 0, T, beam, blank))


def test_small_vocab_long_inputs_many_seeds():
    """V = 3..5, T = 300..500: prefixes drop out of the beam and come back -- a non-canonical node scheme duplicates them."""
    rng = np.random.default_rng(11)
    B = 24
    V = rng.integers(3, 6, B)
    T = rng.integers(300, 501, B)
    beam = rng.integers(2, 9, B)
    for bm in sorted(set(beam.tolist())):
        sel = [b for b in range(B) if beam[b] == bm]
        Tm = int(T[sel].max())
        for Vv in sorted(set(V[sel].tolist())):
            sub = [b for b in sel if V[b] == Vv]
            k = min(bm, Vv)
            x = torch.from_numpy(rng.normal(0, 1.5, (len(sub), Tm, Vv)).astype(np.float32))
            lp, ix = _topk(x, k)
            nb = _device_search(lp, ix, [int(T[b]) for b in sub], int(bm))
            for i, b in enumerate(sub):
                _same_hyps(_hyps(nb, i), _host(lp, ix, i, int(T[b]), int(bm)))


# ------------------------------------------------------------------------------------------------ 3. edge cases
def test_edge_cases():
    from m3asr.decode import CtcBeamSearch
    from m3asr._lib import M3Error
    # one frame, blank best
    lp0 = torch.log(torch.tensor([[[0.6, 0.1, 0.3]]]))
    s = CtcBeamSearch(1, 3, 4)
    s.advance(lp0.cuda(), torch.tensor([1]))
    got = s.nbest()[0]
    assert got[0][0] == () and got[1][0] == (2,)
    lp, ix = _topk(lp0, 3)
    _same_hyps(got, _host(lp, ix, 0, 1, 3))
    # all blank; repeats with and without a separating blank
    for seq in ([0, 0, 0, 0], [1, 1, 0, 1, 1], [2, 2, 2]):
        x = torch.full((1, len(seq), 4), -4.0)
        x[0, torch.arange(len(seq)), torch.tensor(seq)] = 4.0
        lp, ix = _topk(x, 3)
        _same_hyps(_hyps(_device_search(lp, ix, [len(seq)], 3), 0), _host(lp, ix, 0, len(seq), 3))
    # T = 0: the empty prefix with score 0
    assert CtcBeamSearch(2, 4, 0).nbest() == [[((), 0.0)], [((), 0.0)]]
    s = CtcBeamSearch(1, 4, 8)
    s.advance(torch.zeros(1, 3, 6, device="cuda"), torch.tensor([0]))
    assert s.nbest() == [[((), 0.0)]]
    for bad in (0, 33):
        with pytest.raises(M3Error):
            CtcBeamSearch(1, bad, 10)


# ------------------------------------------------------------------------------------------------ 4. batched, ragged
def test_batched_ragged_equals_per_utterance_host():
    from m3asr.decode import CtcBeamSearch
    B, T, V, beam = 16, 125, 1434, 10
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T, V, generator=g) * 2.5
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[0], lens[1], lens[2] = 0, 1, T
    s = CtcBeamSearch(B, beam, T)
    s.advance(x.cuda(), lens.cuda())
    got = s.nbest()
    lp, ix = _topk(x, beam)
    for b in range(B):
        want = _host(lp, ix, b, int(lens[b]), beam) if lens[b] > 0 else [((), 0.0)]
        _same_hyps(got[b], want)


# ------------------------------------------------------------------------------------------------ 5. resumable
def test_chunked_advances_are_bit_identical():
    B, T, V, beam = 5, 120, 50, 8
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, V, generator=g) * 2.0
    lens = [120, 97, 1, 64, 0]
    lp, ix = _topk(x, beam)
    one = _device_search(lp, ix, lens, beam)
    rng = np.random.default_rng(3)
    rand = []
    while sum(rand) < T:
        rand.append(int(min(rng.integers(0, 20), T - sum(rand))))
    for size in (1, 7, 16, None):
        chunks = rand if size is None else [min(size, T - i) for i in range(0, T, size)]
        got = _device_search(lp, ix, lens, beam, chunks=chunks)
        for a, b in zip(got, one):
            assert torch.equal(a, b), size


def test_reset_and_independent_states():
    from m3asr.decode import CtcBeamSearch
    g = torch.Generator().manual_seed(6)
    xa, xb = (torch.randn(2, 40, 30, generator=g).cuda() * 2 for _ in range(2))
    la = torch.tensor([40, 33])
    lb = torch.tensor([25, 40])
    want_a = CtcBeamSearch(2, 5, 40)
    want_a.advance(xa, la)
    want_b = CtcBeamSearch(2, 5, 40)
    want_b.advance(xb, lb)
    sa, sb = CtcBeamSearch(2, 5, 40), CtcBeamSearch(2, 5, 40)
    sa.advance(xb, lb)                          # something else first, then reset
    sa.reset()
    for t0 in range(0, 40, 8):                  # alternate the two searches chunk by chunk
        for s, x, ln in ((sa, xa, la), (sb, xb, lb)):
            s.advance(x[:, t0:t0 + 8], (ln - t0).clamp(0, 8))
    assert sa.nbest() == want_a.nbest()
    assert sb.nbest() == want_b.nbest()


# ------------------------------------------------------------------------------------------------ 6. overflow
def test_overflow_is_reported_not_written():
    from m3asr import ops
    from m3asr._lib import M3Error
    from m3asr.decode import CtcBeamSearch
    B, beam, F, V = 3, 4, 10, 20
    desc = ops.ctc_beam_desc(B, beam, F, 0)
    n = ops.ctc_beam_state_size(desc)
    G = 4096
    buf = torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    state = buf[G:G + n]
    ops.ctc_beam_reset(desc, state)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 8, V, generator=g).cuda()
    lp, ix = ops.ctc_topk(x, beam)
    ops.ctc_beam_advance(desc, state, lp, ix, torch.tensor([8, 8, 2], dtype=torch.int32, device="cuda"))
    ops.ctc_beam_advance(desc, state, lp, ix, torch.tensor([3, 2, 8], dtype=torch.int32, device="cuda"))  # 11 > 10 for b = 0
    _, _, _, nh = ops.ctc_beam_nbest(desc, state)
    assert nh.cpu().tolist()[0] == -1 and nh.cpu().tolist()[1] > 0 and nh.cpu().tolist()[2] > 0
    ops.ctc_beam_advance(desc, state, lp, ix, torch.tensor([1, 0, 0], dtype=torch.int32, device="cuda"))  # sticky
    assert ops.ctc_beam_nbest(desc, state)[3].cpu().tolist()[0] == -1
    assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + n:] == 0xA5).all())
    s = CtcBeamSearch(1, 3, 4)
    s.advance(x[:1, :5].contiguous(), torch.tensor([5]))
    with pytest.raises(M3Error):
        s.nbest()
    # the streaming greedy search: same contract
    gd = ops.ctc_greedy_stream_desc(B, F, 0)
    gn = ops.ctc_greedy_stream_state_size(gd)
    gbuf = torch.full((gn + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    gstate = gbuf[G:G + gn]
    ops.ctc_greedy_stream_reset(gd, gstate)
    ops.ctc_greedy_stream_advance(gd, gstate, x, torch.tensor([8, 8, 8], dtype=torch.int32, device="cuda"))
    ops.ctc_greedy_stream_advance(gd, gstate, x, torch.tensor([8, 2, 0], dtype=torch.int32, device="cuda"))
    assert ops.ctc_greedy_stream_tokens(gd, gstate)[1].cpu().tolist()[0] == -1
    assert bool((gbuf[:G] == 0x5A).all()) and bool((gbuf[G + gn:] == 0x5A).all())


def test_streaming_greedy_equals_greedy_on_concatenation():
    from m3asr import ops
    B, T, V = 4, 90, 12
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, T, V, generator=g)
    x[:, ::3, 0] += 2.0
    lens = torch.tensor([90, 45, 1, 0])
    gd = ops.ctc_greedy_stream_desc(B, T, 0)
    st = torch.empty(ops.ctc_greedy_stream_state_size(gd), dtype=torch.uint8, device="cuda")
    ops.ctc_greedy_stream_reset(gd, st)
    xc = x.cuda()
    for t0 in range(0, T, 13):
        c = min(13, T - t0)
        ops.ctc_greedy_stream_advance(gd, st, xc[:, t0:t0 + c].contiguous(),
                                      (lens - t0).clamp(0, c).to(torch.int32).cuda())
    toks, n = ops.ctc_greedy_stream_tokens(gd, st)
    _, wt, wn = ops.ctc_greedy(xc, lens.to(torch.int32).cuda(), 0)
    assert torch.equal(n.cpu(), wn.cpu())
    assert torch.equal(toks.cpu()[:, :T], wt.cpu())


# ------------------------------------------------------------------------------------------------ 7 / 8. on the engine
def _engine(left):
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=16,
                        num_decoding_left_chunks=left)
    return Engine.from_state_dict(cfg, make_weights(cfg, seed=41), packed_rows=False)


@pytest.mark.parametrize("left", [-1, 2])
def test_chunked_ctc_decoder(left):
    from m3asr.decode import CtcDecoder
    eng = _engine(left)
    dec = CtcDecoder(eng, blank_idx=0)
    g = torch.Generator().manual_seed(9)
    feat = torch.rand(3, 200, eng.cfg.input_dim, generator=g)
    fl = torch.tensor([200, 90, 131], dtype=torch.int32)
    res = dec.forward(feat, fl)
    logits, out_lens = res["out_nosm"].cpu(), res["out_lens"].cpu()
    assert dec.ctc_greedy_search(feat, fl, 16, left) == ref.ctc_greedy_search(logits.numpy(), out_lens.numpy(), 0)
    hyps, _ = dec.batch_prefix_beam_search(feat, fl, 5, 16, left)
    for b in range(3):
        want = ref.ctc_prefix_beam_search(logits[b, :int(out_lens[b])].numpy(), 5, 0)
        assert [p for p, _ in hyps[b]] == [p for p, _ in want]
        np.testing.assert_allclose([s for _, s in hyps[b]], [s for _, s in want], rtol=0, atol=1e-4)
    for bad in ((8, left), (16, 3 if left != 3 else 1)):
        with pytest.raises(NotImplementedError):
            dec.ctc_greedy_search(feat, fl, *bad)
        with pytest.raises(NotImplementedError):
            dec.batch_prefix_beam_search(feat, fl, 5, *bad)


def test_streaming_decoder_end_to_end():
    from m3asr import ops
    from m3asr.config import subsampled_len
    from m3asr.decode import StreamingCtcDecoder
    eng = _engine(2)
    lengths = [333, 206, 64, 150]
    B, c = len(lengths), 16
    g = torch.Generator().manual_seed(10)
    feat = torch.rand(B, max(lengths), eng.cfg.input_dim, generator=g)
    fl = torch.tensor(lengths, dtype=torch.int32)
    T = feat.shape[1]
    Tp = subsampled_len(T)
    beam = 6
    dec = StreamingCtcDecoder(eng.streaming(B, Tp), beam)
    st = dec.st
    # chunk by chunk by hand: the greedy partial after every chunk against m3_ctc_greedy on the frames so far
    n_chunks = -(-Tp // c)
    padded = torch.zeros(B, max(T, 4 * c * n_chunks + 3), feat.shape[2])
    padded[:, :T] = feat
    total = torch.tensor([subsampled_len(v) if v >= 7 else 0 for v in lengths])
    dec.reset()
    seen = []
    for n in range(n_chunks):
        left = (fl.long() - 4 * c * n).clamp(min=0, max=st.window)
        left = torch.where(left >= 7, left, torch.zeros_like(left))
        lg = dec.step(padded[:, 4 * c * n: 4 * c * n + st.window], left)
        eng.stream.synchronize()
        seen.append(lg.clone())
        so_far = (total - 0).clamp(max=(n + 1) * c).to(torch.int32)
        best, greedy = dec.partial()
        _, wt, wn = ops.ctc_greedy(torch.cat(seen, 1).contiguous(), so_far.cuda(), 0)
        wt, wn = wt.cpu(), wn.cpu().tolist()
        assert greedy == [wt[b, :wn[b]].tolist() for b in range(B)], n
        assert len(best) == B
    stepped = dec.finish()
    # after the last chunk: the n-best against the host routine on StreamingEncoder.decode's logits
    full = st.decode(feat, fl)
    lp, ix = ops.ctc_topk(full.contiguous(), beam)
    for b in range(B):
        want = _host(lp, ix, b, int(total[b]), beam) if total[b] > 0 else [((), 0.0)]
        _same_hyps(stepped[b], want)
    assert dec.decode(feat, fl) == stepped
    _, wt, wn = ops.ctc_greedy(full.contiguous(), total.to(torch.int32).cuda(), 0)
    wt, wn = wt.cpu(), wn.cpu().tolist()
    assert dec.greedy() == [wt[b, :wn[b]].tolist() for b in range(B)]
