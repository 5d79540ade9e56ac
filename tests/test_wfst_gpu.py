"""The device WFST search (m3_wfst_search_*, csrc/ctc_wfst.hip) against the host restatement of its contract
(tests/wfst_ref.py, pinned on the CPU by tests/test_wfst_host.py): words, word frames, cost bits, reached_final and status
must be equal, for the final and for the partial result.  The random cases are those of tests/wfst_cases.py, which the CPU
tier shows to exercise the beam cut, the max_active cut at a cost tie, an epsilon winner over an emitting one and a dead search.
"""
import math

import numpy as np
import pytest
import torch

import guarded as G
import wfst_cases as WC
import wfst_ref as R

pytestmark = pytest.mark.gpu

INF = math.inf


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _search(g, B, max_frames, beam, max_active, **kw):
    from m3asr.wfst import CtcWfstSearch
    if g.dev is None:
        g.to("cuda")
    return CtcWfstSearch(g, B, max_frames, beam=beam, max_active=max_active, **kw)


def _results(search, final=True, out=None):
    words, frames, n_words, cost, flags, status = (t.cpu() for t in search.result_tensors(final, out))
    res = []
    for b in range(search.B):
        n = int(n_words[b])
        assert bool((words[b, max(n, 0):] == -1).all()) and bool((frames[b, max(n, 0):] == -1).all())
        res.append(dict(words=words[b, :max(n, 0)].tolist(), frames=frames[b, :max(n, 0)].tolist(), n_words=n, cost=float(cost[b]),
                        reached_final=int(flags[b]), status=int(status[b])))
    return res


def _same(got, want, what):
    assert got["status"] == want["status"], (what, got, want)
    assert got["n_words"] == want["n_words"] and got["words"] == want["words"], (what, got, want)
    assert got["frames"] == want["frames"], (what, got, want)
    assert _bits(got["cost"]) == _bits(want["cost"]), (what, got, want)
    assert got["reached_final"] == want["reached_final"], (what, got, want)


def _logp(rows, T=None):
    """(1, T, V) device log-probabilities from host rows, padded with NaN frames that must not be read"""
    rows = np.asarray(rows, dtype=np.float32)
    T = len(rows) if T is None else T
    x = np.full((1, max(T, 1), rows.shape[1]), np.nan, dtype=np.float32)
    x[0, :len(rows)] = rows
    return torch.from_numpy(x).cuda()


@pytest.mark.parametrize("seed", WC.RANDOM_SEEDS)
def test_random_graphs_equal_the_restatement(seed):
    c = WC.random_case(seed)
    g, logp = c["graph"], c["logp"]
    T = len(logp)
    ref = R.RefSearch(g, c["beam"], c["max_active"]).advance(logp)
    s = _search(g, 1, T, c["beam"], c["max_active"])
    s.advance(_logp(logp), [T], log_softmax=False)
    _same(_results(s)[0], ref.result(True), "final")
    _same(_results(s, final=False)[0], ref.result(False), "partial")
    # a second scale and, every frame a chunk of its own, the partial result at every frame boundary
    ref = R.RefSearch(g, c["beam"], c["max_active"], acoustic_scale=0.5)
    s = _search(g, 1, T, c["beam"], c["max_active"], acoustic_scale=0.5)
    for t in range(min(T, 12)):
        ref.advance(logp[t:t + 1])
        s.advance(_logp(logp[t:t + 1]), [1], log_softmax=False)
        _same(_results(s, final=False)[0], ref.result(False), "partial after frame %d" % t)
    _same(_results(s)[0], ref.result(True), "final after %d frames" % min(T, 12))


@pytest.mark.parametrize("fan,max_active", [(1500, None), (1500, 1100), (1500, 1024), (62, 40), (63, 40), (64, 64), (64, 63)])
def test_size_boundaries(fan, max_active):
    """More live states than the work-group has threads (1501), and live counts of 63, 64 and 65: the strided loops, the
    wave-per-token expansion of the start state's `fan` arcs and the radix select across those sizes, at frequent cost ties."""
    g = WC.wide_graph(fan)
    T, ma = 6, g.n_states if max_active is None else max_active
    logp = WC.flat_logp(T, g.vocab_size, seed=fan)
    ref = R.RefSearch(g, INF, ma).advance(logp)
    assert ref.max_live == fan + 1 and (max_active is None or "max_active_tie" in ref.fired)
    s = _search(g, 1, T, INF, ma)
    s.advance(_logp(logp), [T], log_softmax=False)
    _same(_results(s)[0], ref.result(True), "final")
    ref4 = R.RefSearch(g, 1.0, ma).advance(logp)
    s = _search(g, 1, T, 1.0, ma)
    s.advance(_logp(logp), [T], log_softmax=False)
    _same(_results(s)[0], ref4.result(True), "final, beam 1")


def test_batch_of_unequal_lengths_chunks_and_slot_reset():
    c = WC.random_case(7)
    g, logp = c["graph"], c["logp"]
    T, V = len(logp), g.vocab_size
    assert T >= 9
    lens = [0, 1, T]
    x = torch.full((3, T, V), float("nan"))
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(logp[:n])
    x = x.cuda()
    want = [R.RefSearch(g, 4.0, 5).advance(logp[:n]).result(True) for n in lens]
    one = _search(g, 3, T, 4.0, 5)
    one.advance(x, lens, log_softmax=False)
    got = _results(one)
    for b in range(3):
        _same(got[b], want[b], "utterance %d" % b)
    for chunk in (1, 7):
        s = _search(g, 3, T, 4.0, 5)
        for t0 in range(0, T, chunk):
            s.advance(x[:, t0:t0 + chunk], [min(max(n - t0, 0), chunk) for n in lens], log_softmax=False)
        for b, r in enumerate(_results(s)):
            _same(r, got[b], "chunks of %d, utterance %d" % (chunk, b))
    # a reset of slot 1 leaves the bytes of slots 0 and 2 alone and restarts slot 1
    n = one.bytes_per_utterance
    before = one.state.clone()
    one.reset(slots=[1])
    after = one.state
    assert torch.equal(after[:n], before[:n]) and torch.equal(after[2 * n:3 * n], before[2 * n:3 * n])
    fresh = _results(one)
    _same(fresh[1], want[0], "slot 1 after its reset")
    _same(fresh[2], want[2], "slot 2 after the reset of slot 1")
    one.advance(x[2:3, :1].expand(3, 1, V).contiguous(), [0, 1, 0], log_softmax=False)
    _same(_results(one)[1], want[1], "slot 1 restarted")


@pytest.mark.parametrize("cap", ["token_cap", "record_cap", "max_frames"])
def test_capacity_overflow_fails_soft_inside_guards(cap):
    c = WC.random_case(10)
    g, logp = c["graph"], c["logp"]
    T = len(logp)
    full = R.RefSearch(g, INF, g.n_states).advance(logp)
    assert full.status == 0 and len(full.records) > 4 and T > 4
    caps = {"token_cap": dict(token_cap=3), "record_cap": dict(record_cap=4), "max_frames": dict(max_frames=T - 2)}[cap]
    want = R.RefSearch(g, INF, g.n_states, **caps).advance(logp).result(True)
    assert want["n_words"] == -1 and want["status"] == {"token_cap": R.TOKEN_CAP, "record_cap": R.RECORD_CAP, "max_frames": R.MAX_FRAMES}[cap]
    s = _search(g, 2, caps.get("max_frames", T), INF, g.n_states, **{k: v for k, v in caps.items() if k != "max_frames"})
    state = G.flat_out((s.state.numel(),), torch.uint8)
    s.state = state.view
    s.reset()
    x = torch.cat([_logp(logp), _logp(logp[:2], T)])
    s.advance(x, [T, 2], log_softmax=False)
    s.advance(x, [T, 0], log_softmax=False)                          # the status is sticky: more frames change nothing
    W = s.max_words
    out = (G.flat_out((2, W), torch.int32), G.flat_out((2, W), torch.int32), G.flat_out((2,), torch.int32),
           G.flat_out((2,), torch.float32), G.flat_out((2,), torch.int32), G.flat_out((2,), torch.int32))
    got = _results(s, out=tuple(o.view for o in out))
    _same(got[0], want, cap)
    state.check("state")
    for o, name in zip(out, ("words", "frames", "n_words", "cost", "flags", "status")):
        o.check(name)
    # the other utterance of the batch is untouched by its neighbour's overflow (unless its own two frames overflow too)
    _same(got[1], R.RefSearch(g, INF, g.n_states, **caps).advance(logp[:2]).result(True), "neighbour")
    with pytest.raises(Exception, match=cap.replace("_", ".")):
        s.result()


def test_lexicon_graph_and_decoder_entry_points():
    from m3asr.wfst import DecodingGraph, wfst_from_logits
    g = DecodingGraph.from_lexicon(WC.TOY_LEXICON, 4, word_costs={2: 0.5}).to("cuda")
    ali = [0, 1, 1, 2, 3, 0, 3, 3, 0, 3, 0, 0, 2, 2, 1, 0]                 # words 2, 3, 4 with blanks and repeats
    logits = torch.from_numpy(WC.peaked_logits(ali, 4))[None].cuda()
    out = wfst_from_logits(logits, [len(ali)], g, beam=8.0, max_active=50, detail=True)[0]
    assert out["words"] == [2, 3, 4] and out["reached_final"] and out["status"] == 0
    from m3asr import ops
    want = R.RefSearch(g, 8.0, 50).advance(ops.log_softmax_bias(logits)[0].cpu().numpy()).result(True)
    assert out["words"] == want["words"] and out["frames"] == want["frames"] and _bits(out["cost"]) == _bits(want["cost"])
    # the same through CtcDecoder.ctc_wfst_search on a tiny engine: every token a word, and a few longer words
    from m3asr.config import EncoderConfig
    from m3asr.decode import CtcDecoder
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig.tiny()
    V = cfg.output_dim
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=3), device="cuda:0")
    dec = CtcDecoder(eng)
    gen = torch.Generator().manual_seed(0)
    feat, fl = torch.randn(2, 40, cfg.input_dim, generator=gen), torch.tensor([40, 29], dtype=torch.int32)
    res = dec.forward(feat, fl)
    greedy = dec.greedy_from_logits(res["out_nosm"], res["out_lens"])
    lex = {t: [[t]] for t in range(1, V)}
    for b, toks in enumerate(greedy):
        if len(toks) >= 2:
            lex[V + b] = [toks[:2]]
    big = DecodingGraph.from_lexicon(lex, V, word_costs={w: 0.25 * (w % 4) for w in lex}).to("cuda")
    got = dec.ctc_wfst_search(feat, fl, big, beam=6.0, max_active=64, detail=True)
    logp = ops.log_softmax_bias(res["out_nosm"]).cpu().numpy()
    for b, n in enumerate(res["out_lens"].cpu().tolist()):
        want = R.RefSearch(big, 6.0, 64).advance(logp[b, :n]).result(True)
        assert got[b]["words"] == want["words"] and got[b]["frames"] == want["frames"], (b, got[b], want)
        assert _bits(got[b]["cost"]) == _bits(want["cost"]) and got[b]["reached_final"] == want["reached_final"] == 1
    assert dec.ctc_wfst_search(feat, fl, big, beam=6.0, max_active=64) == [r["words"] for r in got]


def test_constructor_refuses_a_state_over_the_byte_budget():
    from m3asr import _lib
    g = WC.random_case(3)["graph"]
    s = _search(g, 4, 10, 4.0, 5)
    assert s.state.numel() == 4 * s.bytes_per_utterance and s.bytes_per_utterance >= 24 * g.n_states
    with pytest.raises(_lib.M3Error, match="max_state_bytes"):
        _search(g, 4, 10, 4.0, 5, max_state_bytes=4 * s.bytes_per_utterance - 1)
    from m3asr.wfst import DecodingGraph
    with pytest.raises(_lib.M3Error, match="not on a device"):
        from m3asr.wfst import CtcWfstSearch
        CtcWfstSearch(DecodingGraph.from_lexicon({1: [1]}, 3), 1, 4)
