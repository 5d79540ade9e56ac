"""Streaming two-pass decoding: the per-slot encoder-memory store (m3_aed_memory_*, csrc/aed_memory.hip),
AttentionRescorer.rescore_rows, StreamingCtcDecoder(rescorer=).rescore(), StreamPool(rescore=True) and
tools/transcribe_stream.py --rescore.

The store's kernels are copies: they must equal a numpy mirror EXACTLY, in guarded memory.  The scores follow the yardstick of
tests/test_aed_rescore_gpu.py: aed_ref in float64 is the truth, e32 the error of aed_ref in float32 on the same inputs, and
the device must lie within max(8 e32, 1e-5) of float64; every comparison prints its error, e32 and the bound before it
asserts (run with -s).  The reference's memory is aed_ref.layer_norm of the rows of the chunk binding's buffer "x" kept by
the test after every step, never what the store returned.  The winner is compared where the float64 reference's two best
final scores lie more than twice the bound apart; FEAT_SEED was picked on the CPU (oracle/encoder_ref.py) so that both
utterances of the shared run do (asserted, never skipped)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_ref
import guarded
from m3asr import ops
from m3asr._lib import M3Error
from m3asr.config import DecoderConfig, EncoderConfig
from m3asr.decode import EndpointConfig, StreamingCtcDecoder
from m3asr.engine import Engine
from m3asr.plan import pack_decoder
from m3asr.serve import RescoredSegment, Segment, StreamPool, WindowBuffer
from m3asr.weights import make_decoder_weights, make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, MAXF, BEAM = 4, 16, 4
CW, RW = 0.5, 0.3
FEAT_SEED = 3
L_FRAMES = 10
LENGTH_RULE = EndpointConfig(rules=((False, 0, L_FRAMES * 40),))      # as tests/test_ctc_endpoint_gpu.py: fires in a slot's third chunk


# ---------------------------------------------------------------- 1. the store's kernels against numpy
class Store:
    """The store on the device (optionally inside guarded memory) next to its numpy mirror."""

    def __init__(self, B, Tc, MF, D, guard):
        self.B, self.Tc, self.MF, self.D, self.guard = B, Tc, MF, D, guard
        self.desc = ops.aed_memory_desc(B, MF, D)
        nbytes = ops.aed_memory_state_size(self.desc)
        assert nbytes % B == 0 and nbytes >= B * MF * D * 4
        self.stride = nbytes // B
        self.gstate = guarded.flat_out((nbytes,), torch.uint8) if guard else None
        self.state = self.gstate.view if guard else torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ops.aed_memory_reset(self.desc, self.state)
        self.rows = [np.zeros((0, D), np.float32) for _ in range(B)]
        self.failed = [False] * B
        self.rng = np.random.default_rng(D)

    def append(self, n_frames):
        """one append of fresh random rows; checks lengths, gathered rows and the idle slots' bytes"""
        x = self.rng.standard_normal((self.B * self.Tc, self.D)).astype(np.float32)
        before = self.state.cpu().clone()
        if self.guard:                                                 # ldx > D, NaN around the operand
            gx = guarded.strided_in(torch.from_numpy(x))
            assert gx.ld > self.D
            xd = gx.view
        else:
            xd = torch.from_numpy(x).cuda()
        ops.aed_memory_append(self.desc, self.state, xd, torch.tensor(n_frames, dtype=torch.int32, device="cuda"))
        idle = []
        for b, n in enumerate(n_frames):
            n = min(max(n, 0), self.Tc)
            if n == 0:
                idle.append(b)
            elif self.failed[b] or self.rows[b].shape[0] + n > self.MF:
                self.failed[b] = True
            else:
                self.rows[b] = np.concatenate([self.rows[b], x[b * self.Tc: b * self.Tc + n]])
        after = self.state.cpu()
        for b in idle:
            assert torch.equal(after[b * self.stride:(b + 1) * self.stride], before[b * self.stride:(b + 1) * self.stride]), b
        self.check()

    def lengths(self):
        return [-1 if f else r.shape[0] for f, r in zip(self.failed, self.rows)]

    def check(self, slots=None):
        slots = list(range(self.B)) if slots is None else slots
        assert ops.aed_memory_lengths(self.desc, self.state).cpu().tolist() == self.lengths()
        want = [self.rows[b] if 0 <= b < self.B and not self.failed[b] else np.zeros((0, self.D), np.float32) for b in slots]
        total = sum(w.shape[0] for w in want)
        lst = torch.tensor(slots, dtype=torch.int32, device="cuda")
        cap = len(slots) * self.MF
        if self.guard:
            gout = guarded.strided_out(cap, self.D)
            assert gout.ld > self.D
            out, row0 = ops.aed_memory_gather(self.desc, self.state, lst, out=gout.view)
            gout.check("gathered rows")
            untouched = gout.untouched().cpu()
            assert bool(untouched[total:].all()) and not bool(untouched[:total].any())      # rows past the total stay unwritten
            self.gstate.check("memory state")
        else:
            out, row0 = ops.aed_memory_gather(self.desc, self.state, lst)
            assert tuple(out.shape) == (cap, self.D)
        assert row0.cpu().tolist() == [0] + list(np.cumsum([w.shape[0] for w in want]))
        assert guarded.same_bits(out[:total].cpu(), torch.from_numpy(np.concatenate(want) if want else np.zeros((0, self.D), np.float32)))


@pytest.mark.parametrize("D,guard", [(32, True), (512, False), (512, True)])
def test_store_kernels_equal_numpy(D, guard):
    """B = 3, T_chunk = 4, max_frames = 12.  Appends (4,0,2), (3,4,0), (4,4,4); overflow of slot 0 at 11 of 12; reset_slots with
    a list that also holds -1 and B; gather in the order (2, 0); negative and too large frame counts."""
    s = Store(3, 4, 12, D, guard)
    for n_frames in ((4, 0, 2), (3, 4, 0), (4, 4, 4)):
        s.append(n_frames)
    assert s.lengths() == [11, 8, 6]
    s.check(slots=[2, 0])
    s.check(slots=[1, 7, 1, -1])                                       # entries outside [0, B) contribute nothing; a slot may repeat
    s.append((4, 0, 0))                                                # 11 + 4 > 12: consumes nothing, reads -1, the others stay
    assert s.lengths() == [-1, 8, 6]
    s.check(slots=[2, 0])                                              # a failed slot contributes 0 rows
    s.append((1, 1, 1))                                                # stays failed although one row would fit
    assert s.lengths() == [-1, 9, 7]
    ops.aed_memory_reset(s.desc, s.state, torch.tensor([0, -1, 3], dtype=torch.int32, device="cuda"))
    s.rows[0], s.failed[0] = np.zeros((0, D), np.float32), False
    s.check()
    s.append((2, 0, 0))                                                # the restarted slot starts at row 0
    assert s.lengths() == [2, 9, 7]
    ops.aed_memory_reset(s.desc, s.state)
    s.rows = [np.zeros((0, D), np.float32) for _ in range(3)]
    s.check()
    s.append((-2, 9, 4))                                               # clamped to [0, T_chunk]
    assert s.lengths() == [0, 4, 4]


def test_store_rejects_what_it_cannot_copy():
    with pytest.raises(M3Error):
        ops.aed_memory_desc(3, 12, 30)                                 # D no multiple of 4
    desc = ops.aed_memory_desc(2, 8, 32)
    state = torch.empty(ops.aed_memory_state_size(desc), dtype=torch.uint8, device="cuda")
    ops.aed_memory_reset(desc, state)
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    wide = torch.zeros(8, 38, device="cuda")
    with pytest.raises(M3Error, match="ldx"):
        ops.aed_memory_append(desc, state, wide[:, :32], n)            # ldx = 38 is no multiple of 4
    wide = torch.zeros(8, 40, device="cuda")
    with pytest.raises(M3Error, match="aligned"):
        ops.aed_memory_append(desc, state, wide[:, 1:33], n)           # 4 bytes off
    with pytest.raises(M3Error, match="state"):
        ops.aed_memory_append(desc, state[:-256], wide[:, :32], n)     # a state that is too small
    with pytest.raises(M3Error, match="ldo"):
        ops.aed_memory_gather(desc, state, n, out=torch.zeros(16, 38, device="cuda")[:, :32])
    assert ops.aed_memory_lengths(desc, state).cpu().tolist() == [0, 0]


# ---------------------------------------------------------------- the model and the shared run
@pytest.fixture(scope="module")
def model():
    """(engine, decoder config, decoder state dict with random after_norm.*, rescorer)"""
    from m3asr.rescore import AttentionRescorer
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=C,
                        num_decoding_left_chunks=2)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=47), packed_rows=False)
    dcfg = DecoderConfig(vocab=cfg.output_dim, dim=cfg.attention_dim, heads=8, linear_units=64, num_blocks=2, r_num_blocks=1)
    sd = make_decoder_weights(dcfg, seed=31)
    g = torch.Generator().manual_seed(31)
    sd["after_norm.weight"] = torch.rand(dcfg.dim, generator=g) + 0.5
    sd["after_norm.bias"] = torch.randn(dcfg.dim, generator=g) * 0.1
    return eng, dcfg, sd, AttentionRescorer(pack_decoder(sd, dcfg), dcfg, "cuda:0")


def _decoder(model, B=2, independent=True, **kw):
    eng, _, _, rescorer = model
    return StreamingCtcDecoder(eng.streaming(B, MAXF, independent=independent), beam=BEAM, rescorer=rescorer, ctc_weight=CW,
                               reverse_weight=RW, **kw)


def _feats(idim):
    """two sessions: 45 frames = two full windows and a short one of 13 frames (2 output frames < c), and 35 = two full"""
    g = torch.Generator().manual_seed(FEAT_SEED)
    return [torch.rand(45, idim, generator=g), torch.rand(35, idim, generator=g)]


def _run_sessions(dec, sessions):
    """sessions: [(slot, first step, frames)].  Every session is pushed whole and ended; slot b is live from its first step
    on while it has a window.  After every step() the rows of the binding's "x" that count are kept.
    -> (kept rows per slot (n, D) on the CPU, n_out sums per slot)"""
    Bn, idim = dec.beam.B, sessions[0][2].shape[1]
    D = dec.st.eng.cfg.attention_dim
    bufs = {}
    for b, _, frames in sessions:
        bufs[b] = WindowBuffer(C, idim)
        bufs[b].push(frames)
        bufs[b].end()
    kept, total = {b: [] for b in bufs}, {b: 0 for b in bufs}
    win = torch.zeros(Bn, 4 * C + 3, idim)
    step = 0
    while True:
        valid = torch.zeros(Bn, dtype=torch.int32)
        for b, first, _ in sessions:
            if step >= first and bufs[b].ready() > 0:
                _, valid[b] = bufs[b].take(out=win[b])
        if not bool(valid.any()):
            if all(bufs[b].drained() for b in bufs):
                break
            step += 1
            continue
        n_out = dec.frames_of(valid)
        dec.step(win, valid)
        dec.st.eng.stream.synchronize()
        x = dec.st.buffer("x").view(Bn * C, D)
        for b in bufs:
            n = int(n_out[b])
            kept[b].append(x[b * C: b * C + n].cpu().clone())
            total[b] += n
        step += 1
        assert step < 50
    return {b: torch.cat(v) for b, v in kept.items()}, total


@pytest.fixture(scope="module")
def shared_run(model):
    """Slot mode, B = 2: session 0 from step 0 (its last window is short: n_out = 2 < c), session 1 two steps later."""
    eng = model[0]
    dec = _decoder(model)
    feats = _feats(eng.cfg.input_dim)
    kept, total = _run_sessions(dec, [(0, 0, feats[0]), (1, 2, feats[1])])
    return dec, kept, total


def _truth(model, rows, hyps):
    """(float64 result, float32 result) of aed_ref: rows = the raw memory rows per utterance, hyps [[(tokens, prior)]]"""
    _, dcfg, sd, _ = model
    out = []
    for dt in (torch.float64, torch.float32):
        w, b = sd["after_norm.weight"].to(dt), sd["after_norm.bias"].to(dt)
        mem = torch.zeros(len(rows), max(max(r.shape[0] for r in rows), 1), dcfg.dim, dtype=dt)
        for u, r in enumerate(rows):
            mem[u, :r.shape[0]] = aed_ref.layer_norm(r.to(dt), w, b)
        out.append(aed_ref.rescore(sd, dcfg, mem, [r.shape[0] for r in rows], hyps, CW, RW, dtype=dt))
    return out


def _compare(what, model, detail, last, rows, nbest, need_winner):
    """detail: the device's pairs per utterance, last: its tensors (att, r_att, final (n, beam), best), rows: the kept memory
    rows, nbest: finish(detail=True) of the same streams.  -> number of utterances whose winner was compared."""
    hyps = []
    for u, (best, scores) in enumerate(detail):
        assert [h[0] for h in scores] == [h[0] for h in nbest[u]], (what, u)
        for h, (_, score, bonus) in zip(scores, nbest[u]):
            assert h[1] == float(np.float32(score) + np.float32(bonus)), (what, u)     # the prior is the search's ranking key
        hyps.append([(h[0], h[1]) for h in scores])
    r64, r32 = _truth(model, rows, hyps)
    bounds = {}
    for key, got in (("att", last["att"]), ("r_att", last["r_att"]), ("final", last["final"])):
        e32 = max([abs(a - b) for u64, u32 in zip(r64, r32) for a, b in zip(u64[key], u32[key])], default=0.0)
        bounds[key] = bound = max(8 * e32, 1e-5)
        err = max([abs(float(got[u, i]) - v) for u, r in enumerate(r64) for i, v in enumerate(r[key])], default=0.0)
        print("%s %s: device err %.3e, e32 %.3e, bound %.3e" % (what, key, err, e32, bound))
        assert all(np.isfinite(float(got[u, i])) for u, r in enumerate(r64) for i in range(len(r[key])))
        assert err <= bound, (what, key, err, bound)
    decided = 0
    for u, r in enumerate(r64):
        for h, a, f in zip(detail[u][1], r["att"], r["final"]):        # the pairs carry the same numbers as the tensors
            assert abs(h[2] - a) <= bounds["att"] and abs(h[3] - f) <= bounds["final"]
        s = sorted(r["final"], reverse=True)
        gap = float("inf") if len(s) < 2 else s[0] - s[1]
        print("%s utterance %d: %d hypotheses, reference top-two final gap %.3e (2 x bound %.3e), best %d" % (
            what, u, len(s), gap, 2 * bounds["final"], r["best"]))
        if need_winner:
            assert len(s) >= 2 and gap > 2 * bounds["final"], "the seed leaves utterance %d without a decided winner" % u
        if gap > 2 * bounds["final"] and len(s) > 0:
            assert int(last["best"][u]) == r["best"] and tuple(detail[u][0]) == tuple(hyps[u][r["best"]][0])
            decided += 1
    return decided


# ---------------------------------------------------------------- 2. the store sees what the encoder wrote
def test_the_store_holds_the_rows_the_encoder_wrote(shared_run):
    dec, kept, total = shared_run
    assert total == {0: 10, 1: 8}
    assert dec.memory_lengths().tolist() == [10, 8]
    rows, row0 = dec.memory()
    dec.st.eng.stream.synchronize()
    assert row0.cpu().tolist() == [0, 10, 18]
    assert guarded.same_bits(rows[:10].cpu(), kept[0]) and guarded.same_bits(rows[10:18].cpu(), kept[1])
    rows, row0 = dec.memory(slots=[1])
    dec.st.eng.stream.synchronize()
    assert row0.cpu().tolist() == [0, 8] and guarded.same_bits(rows[:8].cpu(), kept[1])
    assert dec.st.positions().tolist() == [10, 8]                     # the frames the encoder itself counts


# ---------------------------------------------------------------- 3. truth
def test_rescore_equals_the_reference_in_slot_mode(model, shared_run):
    dec, kept, _ = shared_run
    detail = dec.rescore(detail=True)
    last = {k: v.cpu() for k, v in dec.rescorer.last.items()}
    assert _compare("slot mode", model, detail, last, [kept[0], kept[1]], dec.finish(detail=True), need_winner=True) == 2
    assert dec.rescore() == [list(best) for best, _ in detail]
    one = dec.rescore(slots=[1], detail=True)                          # one listed stream: another row count, same truth
    last = {k: v.cpu() for k, v in dec.rescorer.last.items()}
    assert _compare("slot mode, stream 1 alone", model, one, last, [kept[1]], dec.finish(slots=[1], detail=True), need_winner=True) == 1


def test_rescore_equals_the_reference_in_lockstep_mode(model):
    """dec.decode(feat, feat_len) then dec.rescore(): the memory rows come from the binding after every chunk of a second,
    hand-driven pass over the same windows (the lockstep engine is deterministic), the lengths are T'(len)."""
    eng = model[0]
    feats = _feats(eng.cfg.input_dim)
    feat = torch.zeros(2, 45, eng.cfg.input_dim)
    feat[0], feat[1, :35] = feats[0], feats[1]
    lens = torch.tensor([45, 35], dtype=torch.int32)
    dec = _decoder(model, independent=False)
    nbest = dec.decode(feat, lens)
    assert dec.memory_lengths().tolist() == [10, 8]
    detail = dec.rescore(detail=True)
    last = {k: v.cpu() for k, v in dec.rescorer.last.items()}
    rows, row0 = dec.memory()
    dec.st.eng.stream.synchronize()
    rows = rows.cpu()
    # the same windows by hand, keeping "x" after every chunk
    dec2 = _decoder(model, independent=False)
    padded = torch.zeros(2, 4 * C * 3 + 3, eng.cfg.input_dim)
    padded[:, :45] = feat
    kept = {0: [], 1: []}
    total = torch.tensor([10, 8])
    for n in range(3):
        left = (lens.long() - 4 * C * n).clamp(min=0, max=4 * C + 3)
        left = torch.where(left >= 7, left, torch.zeros_like(left))
        n_out = (total - n * C).clamp(min=0, max=C)
        dec2.step(padded[:, 4 * C * n: 4 * C * n + 4 * C + 3].to(eng.device), left, n_out)
        eng.stream.synchronize()
        x = dec2.st.buffer("x").view(2 * C, -1)
        for b in (0, 1):
            kept[b].append(x[b * C: b * C + int(n_out[b])].cpu().clone())
    kept = [torch.cat(kept[0]), torch.cat(kept[1])]
    assert guarded.same_bits(rows[:10], kept[0]) and guarded.same_bits(rows[10:18], kept[1])
    assert [[(h[0], h[1]) for h in u] for u in dec.finish(detail=True)] == nbest
    _compare("lockstep", model, detail, last, kept, dec.finish(detail=True), need_winner=True)


# ---------------------------------------------------------------- 4. slot independence, bit for bit
def test_a_session_scores_the_same_bits_in_either_slot(model):
    eng = model[0]
    feat = _feats(eng.cfg.input_dim)[0]
    got = []
    for b in (0, 1):
        dec = _decoder(model)
        _run_sessions(dec, [(b, 0, feat)])
        detail = dec.rescore(detail=True)                              # both streams listed: the idle one holds no memory
        last = {k: v.cpu() for k, v in dec.rescorer.last.items()}
        assert detail[1 - b] == ((), []) and int(last["best"][1 - b]) == -1
        assert len(detail[b][1]) >= 2 and bool(torch.isfinite(last["final"][b, :len(detail[b][1])]).all())
        got.append((detail[b], {k: last[k][b] for k in ("att", "r_att", "final", "best")}))
    assert got[0][0] == got[1][0]
    for k in ("att", "r_att", "final", "best"):
        assert guarded.same_bits(got[0][1][k], got[1][1][k]), k


# ---------------------------------------------------------------- 5. the pool
def _alone(dec, b, frames):
    """A fresh session in slot b of `dec`, fed exactly `frames` (never ended) -> (n-best, EndpointInfo, kept "x" rows)."""
    dec.reset(slots=[b])
    buf = WindowBuffer(C, frames.shape[1])
    buf.push(frames)
    win = torch.zeros(dec.beam.B, 4 * C + 3, frames.shape[1])
    kept = [torch.zeros(0, dec.st.eng.cfg.attention_dim)]
    while buf.ready() > 0:
        valid = torch.zeros(dec.beam.B, dtype=torch.int32)
        _, valid[b] = buf.take(out=win[b])
        n = int(dec.frames_of(valid)[b])
        dec.step(win, valid)
        dec.st.eng.stream.synchronize()
        kept.append(dec.st.buffer("x").view(dec.beam.B * C, -1)[b * C: b * C + n].cpu().clone())
    return dec.finish(slots=[b])[0], dec.endpoints(slots=[b])[0], torch.cat(kept)


def _check_pair(what, model, pair, rows, nbest):
    """one rescored pair (best, scores) against the float64 reference on `rows`; -> 1 if the winner was decided and compared"""
    n, beam = len(pair[1]), BEAM
    last = {k: torch.full((1, beam), float("-inf")) for k in ("att", "final")}
    for i, h in enumerate(pair[1]):
        last["att"][0, i], last["final"][0, i] = h[2], h[3]
    _, dcfg, sd, _ = model
    hyps = [[(h[0], h[1]) for h in pair[1]]]
    assert [h[0] for h in pair[1]] == [h[0] for h in nbest] and [h[1] for h in pair[1]] == [float(np.float32(h[1])) for h in nbest]
    r64, r32 = _truth(model, [rows], hyps)
    bound = {}
    for key in ("att", "final"):
        e32 = max([abs(a - b) for a, b in zip(r64[0][key], r32[0][key])], default=0.0)
        bound[key] = max(8 * e32, 1e-5)
        err = max([abs(float(last[key][0, i]) - v) for i, v in enumerate(r64[0][key])], default=0.0)
        print("%s %s: device err %.3e, e32 %.3e, bound %.3e" % (what, key, err, e32, bound[key]))
        assert err <= bound[key], (what, key, err, bound[key])
    s = sorted(r64[0]["final"], reverse=True)
    gap = float("inf") if len(s) < 2 else s[0] - s[1]
    print("%s: %d hypotheses, reference top-two final gap %.3e (2 x bound %.3e)" % (what, n, gap, 2 * bound["final"]))
    if n > 0 and gap > 2 * bound["final"]:
        assert tuple(pair[0]) == tuple(hyps[0][r64[0]["best"]][0])
        return 1
    return 0


def test_pool_files_rescored_segments(model):
    """The schedule of test_a_long_stream_is_cut_into_segments_that_equal_fresh_sessions with rescore=True: the first five
    fields are what that test computes from fresh sessions, best / scores follow the float64 reference on the fresh session's
    memory (which includes the frames of the firing chunk behind the endpoint: 12 rows for an endpoint at frame 9)."""
    eng = model[0]
    idim = eng.cfg.input_dim
    g = torch.Generator().manual_seed(21)
    feats = [torch.rand(4 * C * 13 + 3, idim, generator=g), torch.rand(4 * C * 11 + 3, idim, generator=g)]
    per_seg = -(-L_FRAMES // C)
    dec = _decoder(model, endpoint=LENGTH_RULE)
    pool = StreamPool(dec, segment=True, rescore=True)
    sid = pool.open()
    assert pool.close(sid, rescored=True) == ((), [])                  # closed before its first chunk
    sids, segs, sent, step = {}, {0: [], 1: []}, {0: 0, 1: 0}, 0
    start, pieces = {0: 0, 1: 2}, [23, 7, 40]
    while True:
        assert step < 100, "schedule does not end"
        for i in (0, 1):
            if step >= start[i] and i not in sids:
                sids[i] = pool.open()
            if i in sids and sent[i] < feats[i].shape[0]:
                n = min(pieces[(step + i) % 3], feats[i].shape[0] - sent[i])
                pool.push(sids[i], feats[i][sent[i]:sent[i] + n])
                sent[i] += n
        live = pool.step()
        for i in sids:
            segs[i] += pool.segments(sids[i])
        if not live and all(sent[i] == feats[i].shape[0] for i in (0, 1)):
            break
        step += 1
    assert [pool.slot_of(sids[i]) for i in (0, 1)] == [0, 1]
    last = [pool.close(sids[i], rescored=True) for i in (0, 1)]
    ref = StreamingCtcDecoder(eng.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE)
    n_seen = decided = 0
    for i, n_segs in ((0, 4), (1, 3)):
        want, mem = [], []
        for j in range(n_segs):
            f0 = 4 * C * per_seg * j
            nbest, info, rows = _alone(ref, i, feats[i][f0:f0 + 4 * C * per_seg + 3])
            assert (info.rule, info.frame, info.frames) == (1, L_FRAMES - 1, L_FRAMES) and rows.shape[0] == per_seg * C
            off = per_seg * C * j
            if len(nbest[0][0]) > 0:
                first = info.first_speech if info.first_speech >= 0 else 0
                lastf = info.last_speech if info.last_speech >= 0 else info.frame
                want.append((1, (off + first) * 40, (off + lastf + 1) * 40, nbest, off + L_FRAMES - 1))
                mem.append(rows)
        assert all(isinstance(s, RescoredSegment) for s in segs[i])
        assert [tuple(s)[:5] for s in segs[i]] == want, (i, segs[i], want)
        assert [tuple(Segment(*s[:5])) for s in segs[i]] == want
        for j, (s, rows) in enumerate(zip(segs[i], mem)):
            decided += _check_pair("pool session %d segment %d" % (i, j), model, (s.best, s.scores), rows, s.nbest)
        n_seen += len(want)
        nbest, info, rows = _alone(ref, i, feats[i][4 * C * per_seg * n_segs:])
        assert info.rule == 0
        decided += _check_pair("pool session %d open segment" % i, model, last[i], rows, nbest)
    assert n_seen >= 4, "the random model decodes nothing: the comparison would be empty"
    print("pool: %d segments with tokens, %d winners decided and compared" % (n_seen, decided))


# ---------------------------------------------------------------- 6. refusals
def test_refusals(model):
    from m3asr.rescore import AttentionRescorer
    eng, dcfg, sd, rescorer = model
    plain = StreamingCtcDecoder(eng.streaming(2, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE)
    assert plain.rescorer is None and not hasattr(plain, "mstate")     # nothing is allocated without a rescorer
    with pytest.raises(M3Error, match="rescorer"):
        plain.rescore()
    with pytest.raises(M3Error, match="rescorer"):
        StreamPool(plain, segment=True, rescore=True)
    with pytest.raises(M3Error, match="rescore=True"):
        pool = StreamPool(plain, segment=True)
        pool.close(pool.open(), rescored=True)
    for other in (DecoderConfig(vocab=dcfg.vocab, dim=256, heads=4, linear_units=64, num_blocks=1),
                  DecoderConfig(vocab=dcfg.vocab - 1, dim=dcfg.dim, heads=8, linear_units=64, num_blocks=1)):
        wrong = AttentionRescorer(pack_decoder(dict(make_decoder_weights(other, seed=1), **{
            "after_norm.weight": torch.ones(other.dim), "after_norm.bias": torch.zeros(other.dim)}), other), other, "cuda:0")
        with pytest.raises(M3Error, match="dim %d / vocab %d" % (other.dim, other.vocab)):
            StreamingCtcDecoder(eng.streaming(2, MAXF, independent=True), beam=BEAM, rescorer=wrong)
    with pytest.raises(M3Error, match="right-to-left"):
        one_way = DecoderConfig(vocab=dcfg.vocab, dim=dcfg.dim, heads=8, linear_units=64, num_blocks=1)
        StreamingCtcDecoder(eng.streaming(2, MAXF, independent=True), beam=BEAM, reverse_weight=0.3, rescorer=AttentionRescorer(
            pack_decoder(dict(make_decoder_weights(one_way, seed=1), **{"after_norm.weight": torch.ones(dcfg.dim),
                                                                       "after_norm.bias": torch.zeros(dcfg.dim)}), one_way), one_way, "cuda:0"))


# ---------------------------------------------------------------- 7. the command line
def test_transcribe_stream_rescore_command_line():
    """--synthetic 3 --rescore, cut every second by a length rule: one rescored line behind every segment line, and the
    token lists parse"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable, "tools/transcribe_stream.py", "--synthetic", "3", "--rescore", "--beam", "4",
                        "--rule", "0,0,1000"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    plain = re.findall(r"^(\d+)-(\d*) ms rule (\d+): ([\d ]*)$", r.stdout, re.M)
    second = re.findall(r"^(\d+)-(\d*) ms rule (\d+) rescored: att=(\S+) final=(\S+) tokens=([\d ]*)$", r.stdout, re.M)
    assert len(plain) >= 2 and [p[:3] for p in plain] == [s[:3] for s in second], r.stdout[-3000:]
    assert plain[-1][2] == "0" and any(p[2] == "1" for p in plain)
    for p, s in zip(plain, second):
        tokens = [int(t) for t in s[5].split()]
        assert all(0 <= t < 1434 for t in tokens)
        if p[3].strip():                                               # something was decoded: the scores are numbers
            assert np.isfinite(float(s[3])) and np.isfinite(float(s[4]))
