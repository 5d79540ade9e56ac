"""CTC blank-frame skipping on the device (m3_wfst_skip_*, csrc/ctc_wfst_skip.hip) against the host restatement of its contract
(tests/wfst_skip_ref.py, pinned on the CPU by tests/test_wfst_skip_host.py): emitted rows bit for bit, counts, the frame map,
the saved row; and CtcWfstSearch(blank_skip=p) against RefSkipSearch -- words, mapped frames, cost bits, reached_final, status.
The random cases are those of tests/wfst_cases.py, on which the CPU tier shows the re-insert rule to fire 61 and 21 times."""
import numpy as np
import pytest
import torch

import guarded as G
import wfst_cases as WC
import wfst_skip_ref as S
from m3asr.ops import wfst_skip_desc, wfst_skip_state_size

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.5, 0.7)
CHUNKINGS = (None, 1, 7)                                                        # None = the whole utterance in one call
HDR = 8                                                                         # header words of an utterance's state


def _bits(x):
    return int(np.float32(x).view(np.uint32))


class Device:
    """The skip state of B utterances on the device and the calls on it."""

    def __init__(self, B, V, blank, max_frames, thr, state=None):
        from m3asr import ops
        self.ops, self.B, self.V, self.max_frames = ops, B, V, max_frames
        self.desc = wfst_skip_desc(B, V, blank, max_frames, float(thr))
        self.bytes = wfst_skip_state_size(self.desc)
        assert self.bytes == B * (-(-(4 * (HDR + V + max_frames)) // 16) * 16)
        self.state = torch.empty(self.bytes, dtype=torch.uint8, device="cuda") if state is None else state
        self.n_kept = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        ops.wfst_skip_reset(self.desc, self.state)

    def select(self, logp, n_frames, out=None):
        """logp (B, Tc, >= V) device view -> (rows emitted per utterance as (k, V) int32 bit arrays, the out tensor)"""
        B, Tc = logp.shape[0], logp.shape[1]
        if out is None:
            out = torch.full((B, Tc + 1, self.V), float("nan"), device="cuda")
        nf = torch.tensor(n_frames, dtype=torch.int32).cuda()
        self.ops.wfst_skip_select(self.desc, self.state, logp, nf, out, self.n_kept)
        k = self.n_kept.cpu().tolist()
        rows = out.cpu().numpy()
        return [rows[b, :k[b], :self.V].view(np.int32) for b in range(B)], out

    def utterance(self, b):
        """(header words, saved row bits, map) of utterance b"""
        words = self.state.cpu().numpy().view(np.int32).reshape(self.B, -1)[b]
        return words[:HDR].tolist(), words[HDR:HDR + self.V], words[HDR + self.V:HDR + self.V + self.max_frames].tolist()

    def same_state(self, b, ref, what):
        hdr, saved, fmap = self.utterance(b)
        assert hdr[0] == ref.last_blank and hdr[1] == ref.last_best and hdr[3:] == [ref.n_seen, ref.n_kept, 0, 0, 0], (what, hdr, vars(ref))
        held = min(ref.n_kept, self.max_frames)
        assert fmap[:held] == ref.map[:held], (what, fmap, ref.map)
        if ref.last_blank:                                                      # the saved row counts only after a skipped frame
            assert hdr[2] == ref.saved_frame and np.array_equal(saved, ref.saved.view(np.int32)), (what, hdr)


def _padded(rows, T=None):
    """(1, T, V) device log-probabilities from host rows, padded with NaN frames that must not be read"""
    rows = np.asarray(rows, dtype=np.float32)
    T = len(rows) if T is None else T
    x = np.full((1, max(T, 1), rows.shape[1]), np.nan, dtype=np.float32)
    x[0, :len(rows)] = rows
    return torch.from_numpy(x).cuda()


def _chunks(T, chunk):
    return [(0, T)] if chunk is None else [(t0, min(chunk, T - t0)) for t0 in range(0, T, chunk)]


@pytest.mark.parametrize("seed", WC.RANDOM_SEEDS)
def test_select_equals_the_restatement(seed):
    logp = WC.random_case(seed)["logp"]
    T, V = logp.shape
    for p in THRESHOLDS:
        thr = S.log_thresh(p)
        for chunk in CHUNKINGS:
            dev, ref = Device(1, V, 0, T, thr), S.SkipState(0)
            for t0, n in _chunks(T, chunk):
                want = S.select(logp[t0:t0 + n], 0, thr, ref)
                (got,), _ = dev.select(_padded(logp[t0:t0 + n], chunk), [n])
                what = "seed %d p %g chunk %s frame %d" % (seed, p, chunk, t0)
                assert got.shape == want.shape and np.array_equal(got, want.view(np.int32)), what
                dev.same_state(0, ref, what)                                    # the saved row too, after a chunk that ends skipped
            seen, kept = (t.cpu().tolist() for t in dev.ops.wfst_skip_counts(dev.desc, dev.state))
            assert (seen, kept) == ([T], [ref.n_kept])


@pytest.mark.parametrize("T", [64, 65, 150])
def test_chunks_longer_than_a_tile(T):
    """The kernel walks a chunk in tiles of 64 frames: a chunk of exactly one tile, of one frame more, and of three tiles with
    skipped rows that come back in a later tile than their own; B = 2, the second utterance shorter."""
    rng = np.random.default_rng(T)
    V, thr = 6, S.log_thresh(0.5)
    logp = WC.random_logp(rng, T, V)
    if T > 65:
        logp[62:64, 0], logp[[61, 64]] = -0.25, -4.0                             # frames 62, 63 (first tile) skipped ...
        logp[61, 3] = logp[64, 3] = -0.25                                        # ... between two frames whose best is token 3
    lens = [T, T - 7]
    x = torch.from_numpy(np.stack([logp, logp])).cuda()
    refs = [S.SkipState(0), S.SkipState(0)]
    want = [S.select(logp[:n], 0, thr, r) for n, r in zip(lens, refs)]
    assert T <= 65 or (refs[0].map.count(63) == 1 and 62 not in refs[0].map and refs[0].map.index(64) == refs[0].map.index(63) + 1)
    dev = Device(2, V, 0, T, thr)
    got, _ = dev.select(x, lens)
    for b in range(2):
        assert np.array_equal(got[b], want[b].view(np.int32)), b
        dev.same_state(b, refs[b], "T = %d, utterance %d" % (T, b))
    dev70, parts = Device(2, V, 0, T, thr), [[], []]
    for t0 in range(0, T, 70):
        c = min(70, T - t0)
        rows, _ = dev70.select(x[:, t0:t0 + c].contiguous(), [min(max(n - t0, 0), c) for n in lens])
        for b in range(2):
            parts[b].append(rows[b])
    for b in range(2):
        assert np.array_equal(np.concatenate(parts[b]), want[b].view(np.int32)), b
        dev70.same_state(b, refs[b], "T = %d in chunks of 70, utterance %d" % (T, b))


def test_batch_of_unequal_lengths_strides_and_slot_reset():
    logp = WC.random_case(7)["logp"]
    T, V = logp.shape
    lens, thr, ld, ld_out = [0, 1, T], S.log_thresh(0.5), V + 3, V + 5
    x = torch.full((3, T, ld), float("nan"))
    for b, n in enumerate(lens):
        x[b, :n, :V] = torch.from_numpy(logp[:n])
    x = x.cuda()
    refs = [S.SkipState(0) for _ in lens]
    want = [S.select(logp[:n], 0, thr, r) for n, r in zip(lens, refs)]
    dev = Device(3, V, 0, T, thr)
    out = torch.full((3, T + 1, ld_out), float("nan"), device="cuda")
    got, _ = dev.select(x[:, :, :V], lens, out[:, :, :V])
    for b in range(3):
        assert np.array_equal(got[b], want[b].view(np.int32)), b
        dev.same_state(b, refs[b], "utterance %d" % b)
        assert bool(torch.isnan(out[b, len(want[b]):]).all()) and bool(torch.isnan(out[b, :, V:]).all())
    # the same in chunks of 7, n_frames above T_chunk and below 0 clamped
    dev7 = Device(3, V, 0, T, thr)
    parts = [[], [], []]
    for t0 in range(0, T, 7):
        c = min(7, T - t0)
        nf = [-3 if n - t0 <= 0 else n - t0 for n in lens]                       # [T - t0 > c is clamped to c]
        rows, _ = dev7.select(x[:, t0:t0 + c, :V].contiguous(), nf)
        for b in range(3):
            parts[b].append(rows[b])
    for b in range(3):
        assert np.array_equal(np.concatenate(parts[b]), want[b].view(np.int32)), b
        dev7.same_state(b, refs[b], "chunks of 7, utterance %d" % b)
    # a reset of slot 1 leaves the bytes of slots 0 and 2 alone and restarts slot 1
    n = dev.bytes // 3
    before = dev.state.clone()
    dev.ops.wfst_skip_reset(dev.desc, dev.state, torch.tensor([1], dtype=torch.int32).cuda())
    assert torch.equal(dev.state[:n], before[:n]) and torch.equal(dev.state[2 * n:], before[2 * n:])
    assert dev.utterance(1)[0] == [0, 0, 0, 0, 0, 0, 0, 0]
    seen, kept = (t.cpu().tolist() for t in dev.ops.wfst_skip_counts(dev.desc, dev.state))
    assert seen == [0, 0, T] and kept == [0, 0, refs[2].n_kept]
    dev.ops.wfst_skip_reset(dev.desc, dev.state, torch.tensor([7, -1], dtype=torch.int32).cuda())   # outside [0, B): skipped
    assert torch.equal(dev.state[:n], before[:n]) and torch.equal(dev.state[2 * n:], before[2 * n:])


def test_long_rows_and_the_argmax_tie():
    """V = 1434: rows longer than a wave's stride of 64, the blank at a column inside the row, and maxima that tie across
    lanes -- the smallest index decides whether a saved row comes back."""
    V, blank, thr = 1434, 700, S.log_thresh(0.5)
    rng = np.random.default_rng(3)
    x = rng.choice(np.array([-4.0, -2.0, -1.0], dtype=np.float32), size=(9, V))
    peak, sure = np.float32(-0.25), np.float32(-0.01)
    x[0, 70] = peak
    x[2, [70, 1400]] = peak                                                     # best = 70 = last_best: frame 1 comes back
    x[4, [1400, 1401]] = peak                                                   # best = 1400 != 70: it does not
    x[6, [1400, 1433]] = peak                                                   # best = 1400 = last_best: frame 5 comes back
    x[7, [blank, 900]] = np.float32(-0.9)                                       # below the threshold, ties with 900: best = blank
    x[[1, 3, 5, 8], blank] = sure
    ref = S.SkipState(blank)
    want = S.select(x, blank, thr, ref)
    assert ref.map == [0, 1, 2, 4, 5, 6, 7] and ref.reinserted == 2 and ref.last_blank == 1 and ref.last_best == blank
    for chunk in (None, 4):
        dev, st, parts = Device(1, V, blank, 9, thr), S.SkipState(blank), []
        for t0, n in _chunks(9, chunk):
            S.select(x[t0:t0 + n], blank, thr, st)
            (got,), _ = dev.select(_padded(x[t0:t0 + n]), [n])
            parts.append(got)
            dev.same_state(0, st, "chunk %s frame %d" % (chunk, t0))
        assert np.array_equal(np.concatenate(parts), want.view(np.int32))
    # NaN entries count as -inf for the argmax and never skip a frame
    y = x.copy()
    y[2, 5], y[1, blank] = np.nan, np.nan
    ref = S.SkipState(blank)
    want = S.select(y, blank, thr, ref)
    dev = Device(1, V, blank, 9, thr)
    (got,), _ = dev.select(_padded(y), [9])
    assert np.array_equal(got, want.view(np.int32)) and ref.map[:3] == [0, 1, 2] and ref.reinserted == 1
    dev.same_state(0, ref, "NaN entries")


def test_nothing_is_written_outside_out_and_the_map():
    """out holds exactly T_chunk + 1 rows and the state is sized for max_frames = 3 while more frames are kept."""
    logp = WC.random_case(10)["logp"]
    T, V = logp.shape
    thr = S.log_thresh(0.7)
    ref = S.SkipState(0)
    want = S.select(logp, 0, thr, ref)
    assert ref.n_kept > 3
    from m3asr import ops
    state = G.flat_out((wfst_skip_state_size(wfst_skip_desc(2, V, 0, 3, float(thr))),), torch.uint8)
    dev = Device(2, V, 0, 3, thr, state=state.view)
    half = T // 2
    # utterance 0: the whole utterance in two calls, the second one taking a row the first saved when there is one;
    # utterance 1: the first frame alone
    for t0, n in ((0, half), (half, T - half)):
        out = G.flat_out((2, n + 1, V), torch.float32)
        x = torch.cat([_padded(logp[t0:t0 + n]), _padded(logp[:1], n)])
        n_kept = G.flat_out((2,), torch.int32)
        dev.n_kept = n_kept.view
        dev.select(x, [n, 1 if t0 == 0 else 0], out.view)
        out.check("out")
        n_kept.check("n_kept")
    state.check("state")
    hdr, _, fmap = dev.utterance(0)
    assert hdr[3:5] == [T, ref.n_kept] and fmap == ref.map[:3]
    seen, kept = (G.flat_out((2,), torch.int32) for _ in range(2))
    ops.wfst_skip_counts(dev.desc, dev.state, (seen.view, kept.view))
    seen.check("seen"), kept.check("kept")
    assert seen.view.cpu().tolist() == [T, 1] and kept.view.cpu().tolist()[0] == ref.n_kept
    # map_frames in place: entries at or beyond n_words, and an utterance with n_words < 0, are left alone
    frames = G.flat_out((2, 6), torch.int32)
    frames.view.copy_(torch.tensor([[0, 2, 3, ref.n_kept, -1, 1], [0, 0, 0, 0, 0, 0]], dtype=torch.int32))
    ops.wfst_skip_map_frames(dev.desc, dev.state, frames.view, torch.tensor([5, -1], dtype=torch.int32).cuda())
    frames.check("frames")
    assert frames.view.cpu().tolist() == [[ref.map[0], ref.map[2], T, T, T, 1], [0, 0, 0, 0, 0, 0]]
    assert S.map_frames([0, 2, 3, ref.n_kept, -1], ref, max_frames=3) == [ref.map[0], ref.map[2], T, T, T]


# ---- end to end: CtcWfstSearch(blank_skip=p) against select + RefSearch + the map
def _results(search, final):
    words, frames, n_words, cost, flags, status = (t.cpu() for t in search.result_tensors(final))
    n = int(n_words[0])
    return dict(words=words[0, :max(n, 0)].tolist(), frames=frames[0, :max(n, 0)].tolist(), n_words=n, cost=float(cost[0]),
                reached_final=int(flags[0]), status=int(status[0]))


def _same(got, want, what):
    assert got["status"] == want["status"], (what, got, want)
    assert got["n_words"] == want["n_words"] and got["words"] == want["words"], (what, got, want)
    assert got["frames"] == want["frames"], (what, got, want)
    assert _bits(got["cost"]) == _bits(want["cost"]) and got["reached_final"] == want["reached_final"], (what, got, want)


@pytest.mark.parametrize("seed", WC.RANDOM_SEEDS)
def test_search_with_blank_skip_equals_the_restatement(seed):
    from m3asr.wfst import CtcWfstSearch
    c = WC.random_case(seed)
    g, logp = c["graph"], c["logp"]
    T = len(logp)
    if g.dev is None:
        g.to("cuda")
    for p in THRESHOLDS:
        ref = S.RefSkipSearch(g, c["beam"], c["max_active"], p, max_frames=T).advance(logp)
        for chunk in CHUNKINGS:
            s = CtcWfstSearch(g, 1, T, beam=c["beam"], max_active=c["max_active"], blank_skip=p)
            for t0, n in _chunks(T, chunk):
                s.advance(_padded(logp[t0:t0 + n], chunk), [n], log_softmax=False)
            what = "seed %d p %g chunk %s" % (seed, p, chunk)
            _same(_results(s, True), ref.result(True), what + " final")
            _same(_results(s, False), ref.result(False), what + " partial")
            assert s.frames() == [ref.frames()], what


def test_max_frames_bounds_the_decoded_frames_and_reset_restarts_both_states():
    from m3asr import _lib
    from m3asr.wfst import CtcWfstSearch
    c = WC.random_case(10)
    g, logp = c["graph"], c["logp"]
    if g.dev is None:
        g.to("cuda")
    T, p = len(logp), 0.7
    full = S.RefSkipSearch(g, np.inf, g.n_states, p).advance(logp)
    n_dec = full.frames()[1]
    assert full.search.status == 0 and 4 < n_dec < T
    tight = S.RefSkipSearch(g, np.inf, g.n_states, p, max_frames=n_dec - 1).advance(logp)
    assert tight.result(True)["status"] == 8 and tight.result(True)["n_words"] == -1
    s = CtcWfstSearch(g, 2, n_dec - 1, beam=np.inf, max_active=g.n_states, blank_skip=p)
    x = torch.cat([_padded(logp), _padded(logp)])
    s.advance(x, [T, T], log_softmax=False)
    _same(_results(s, True), tight.result(True), "max_frames = decoded - 1")
    with pytest.raises(_lib.M3Error, match="max.frames"):
        s.result()
    roomy = CtcWfstSearch(g, 2, n_dec, beam=np.inf, max_active=g.n_states, blank_skip=p)   # T frames seen, n_dec decoded: fits
    roomy.advance(x, [T, 3], log_softmax=False)
    _same(_results(roomy, True), full.result(True), "max_frames = decoded")
    roomy.reset(slots=[0])
    assert roomy.frames()[0] == (0, 0) and roomy.frames()[1][0] == 3
    roomy.advance(x, [T, 0], log_softmax=False)
    _same(_results(roomy, True), full.result(True), "after the slot's reset")
    plain = CtcWfstSearch(g, 1, T, beam=np.inf, max_active=g.n_states)
    assert plain.skip is None and not hasattr(plain, "skip_state")
    with pytest.raises(_lib.M3Error, match="blank_skip"):
        plain.frames()


def test_toy_lexicon_through_the_decoder_entry_point():
    from m3asr import ops
    from m3asr.wfst import DecodingGraph, wfst_from_logits
    g = DecodingGraph.from_lexicon(WC.TOY_LEXICON, 5).to("cuda")
    ali = [1, 2, 0, 0, 3, 0, 3, 0, 2, 1]
    logits = torch.from_numpy(WC.peaked_logits(ali, 5, 8.0))[None].cuda()
    out = wfst_from_logits(logits, [len(ali)], g, beam=8.0, max_active=50, blank_skip=0.98, detail=True)[0]
    logp = ops.log_softmax_bias(logits)[0].cpu().numpy()
    want = S.RefSkipSearch(g, 8.0, 50, 0.98).advance(logp).result(True)
    assert out["words"] == want["words"] == [1, 3, 4] and out["frames"] == want["frames"] and _bits(out["cost"]) == _bits(want["cost"])
    assert out["reached_final"] == want["reached_final"] == 1 and max(out["frames"]) > 6       # real frames, not decoded ones
