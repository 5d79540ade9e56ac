"""Slot mode of the chunk-by-chunk engine: the B streams of one streaming state start, pause and end independently
(m3_engine_forward_chunk_slots, m3_engine_stream_reset_slots, m3_engine_stream_positions; StreamingEncoder(independent=True),
StreamingCtcDecoder / CtcBeamSearch with slots=..., m3asr.serve.StreamPool).

The yardstick throughout is the LOCKSTEP path at the same B (tests/test_streaming_gpu.py ties that one to the full-utterance
forward and through it to the CPU oracle and the reference-forward fixtures).  Same B = same kernels (they are chosen by row
count B c).  In fp32 a row's result does not depend on which other rows share the launch or where the stream stands in
wall-clock steps, so the comparisons are torch.equal / exact equality of n-best tokens and scores.  Reference inputs carry
zeros behind every utterance's last frame, which is what a slot's window holds behind its real frames.
"""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3asr._lib import M3Error
from m3asr.config import EncoderConfig, subsampled_len
from m3asr.decode import StreamingCtcDecoder
from m3asr.engine import Engine
from m3asr.serve import StreamPool, WindowBuffer
from m3asr.weights import make_weights


def _cfg(chunk, left, **kw):
    base = dict(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=chunk,
                num_decoding_left_chunks=left)
    base.update(kw)
    return EncoderConfig(**base)


def _utts(lengths, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, cfg.input_dim, generator=g) for n in lengths]


def _batch(utts, idim):
    """Utterances side by side, zeros behind each one's end; an empty slot is an utterance of length 0."""
    T = max(max(int(u.shape[0]) for u in utts), 7)
    feat = torch.zeros(len(utts), T, idim)
    for b, u in enumerate(utts):
        feat[b, :u.shape[0]] = u
    return feat, torch.tensor([int(u.shape[0]) for u in utts], dtype=torch.int32)


def _out_len(n):
    return subsampled_len(n) if n >= 7 else 0


def _run(eng, stepper, B, c, idim, plan, reset, pauses=(), on_done=None):
    """Drive a slot-mode encoder / decoder by hand.  plan: [(slot, first step it may start at, feat (T, idim))]; the utterances
    of a slot run one after the other (a reused slot is restarted first); pauses: {(slot, step)} where a ready slot stays idle.
    -> per plan entry the concatenated logits of its chunks (n chunks * c, V)."""
    queue = {b: [(i, s0, f) for i, (sl, s0, f) in enumerate(plan) if sl == b] for b in range(B)}
    active, used, outs = {b: None for b in range(B)}, set(), {i: [] for i in range(len(plan))}
    win, step = torch.zeros(B, 4 * c + 3, idim), 0
    while any(active.values()) or any(queue.values()):
        assert step < 400, "schedule does not end"
        valid, live = torch.zeros(B, dtype=torch.int32), []
        for b in range(B):
            if active[b] is None and queue[b] and step >= queue[b][0][1]:
                i, _, f = queue[b].pop(0)
                if b in used:
                    reset([b])
                used.add(b)
                wb = WindowBuffer(c, idim)
                wb.push(f)
                wb.end()
                active[b] = (i, wb)
            if active[b] is not None and (b, step) not in pauses and active[b][1].ready():
                _, v = active[b][1].take(out=win[b])
                valid[b] = v
                live.append(b)
        if live:
            lg = stepper(win, valid)
            eng.stream.synchronize()
            for b in live:
                outs[active[b][0]].append(lg[b].cpu())
        for b in range(B):
            if active[b] is not None and active[b][1].drained():
                if on_done is not None:
                    on_done(active[b][0], b)
                active[b] = None
        step += 1
    V = eng.cfg.output_dim
    return [torch.cat(outs[i]) if outs[i] else torch.zeros(0, V) for i in range(len(plan))]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("chunk,left,lengths", [(16, 2, [333, 206, 64, 150]), (12, -1, [206, 100, 57])])
def test_all_slots_together_equals_lockstep_bitwise(dtype, chunk, left, lengths):
    """1. Every slot started on the same call: the same rows through the same launches as lockstep -> the same bits, fp32
    and bf16, ragged lengths (one utterance ends early), eagerly, capturing and replaying."""
    cfg = _cfg(chunk, left, weight_dtype=dtype)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=41), packed_rows=False, bf16_activations=False)
    feat, fl = _batch(_utts(lengths, cfg, 8), cfg.input_dim)
    Tp = subsampled_len(max(lengths))
    lock, slot = eng.streaming(len(lengths), Tp), eng.streaming(len(lengths), Tp, independent=True)
    for use_graph in (False, True, True):
        want = lock.decode(feat, fl, use_graph=use_graph).cpu()
        got = slot.decode(feat, fl, use_graph=use_graph).cpu()
        assert torch.equal(got, want), (use_graph, float((got - want).abs().max()))
        assert slot.positions().tolist() == [_out_len(n) for n in lengths]
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("chunk,left", [(16, 2), (8, -1), (12, 1)])
def test_staggered_starts_equal_lockstep(chunk, left):
    """2. B = 3, streams begin at steps 0, 2 and 5 (idle before), different lengths: every slot's concatenated logits equal
    its rows of a lockstep decode of the three utterances; the whole run captures exactly one graph."""
    cfg = _cfg(chunk, left)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=42), packed_rows=False)
    lengths = [290, 333, 150]
    utts = _utts(lengths, cfg, 9)
    feat, fl = _batch(utts, cfg.input_dim)
    Tp = subsampled_len(max(lengths))
    want = eng.streaming(3, Tp).decode(feat, fl).cpu()
    slot = eng.streaming(3, Tp, independent=True)
    before = eng.num_captures()
    got = _run(eng, slot.step, 3, chunk, cfg.input_dim, [(0, 0, utts[0]), (1, 2, utts[1]), (2, 5, utts[2])], slot.reset)
    assert eng.num_captures() == before + 1
    for b, n in enumerate(lengths):
        k = _out_len(n)
        assert got[b].shape[0] >= k > 0
        assert torch.equal(got[b][:k], want[b, :k]), (b, float((got[b][:k] - want[b, :k]).abs().max()))
    assert slot.positions().tolist() == [_out_len(n) for n in lengths]


@pytest.mark.parametrize("len_c", [380, 90])
def test_slot_reuse_after_partial_reset(len_c):
    """3. B = 2, ring history.  Slot 0 decodes A to its end and is restarted alone while slot 1 is in the middle of B; slot 0
    then decodes C (longer / shorter than A).  C and B equal their lockstep results.  A restart that only zeroed the counter
    and left A's conv cache in place fails on C's first chunk (its first K-1 depthwise taps would read A's last frames
    instead of the left_fill row); the K / V history is deliberately NOT cleared by the restart."""
    cfg = _cfg(16, 2)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=43), packed_rows=False)
    A, Bu, Cu = _utts([170, 640, len_c], cfg, 10)
    Tp = subsampled_len(640)
    lock = eng.streaming(2, Tp)
    want_ab = lock.decode(*_batch([A, Bu], cfg.input_dim)).cpu()
    want_cb = lock.decode(*_batch([Cu, Bu], cfg.input_dim)).cpu()
    slot = eng.streaming(2, Tp, independent=True)
    resets = []

    def reset(slots):
        resets.append((list(slots), slot.positions().tolist()))
        slot.reset(slots=slots)

    got = _run(eng, slot.step, 2, 16, cfg.input_dim, [(0, 0, A), (1, 1, Bu), (0, 0, Cu)], reset)
    assert len(resets) == 1 and resets[0][0] == [0]
    assert resets[0][1][0] == _out_len(170) and 0 < resets[0][1][1] < _out_len(640)      # B was in the middle
    ka, kb, kc = _out_len(170), _out_len(640), _out_len(len_c)
    assert torch.equal(got[0][:ka], want_ab[0, :ka])
    assert torch.equal(got[1][:kb], want_ab[1, :kb]) and torch.equal(got[1][:kb], want_cb[1, :kb])
    assert torch.equal(got[2][:kc], want_cb[0, :kc]), float((got[2][:kc] - want_cb[0, :kc]).abs().max())
    assert not torch.equal(got[2][:16], got[0][:16])


@pytest.mark.parametrize("chunk,left", [(16, 2), (8, -1)])
def test_a_pause_changes_nothing(chunk, left):
    """4. A slot that is idle for two steps in the middle of its utterance goes on as if nothing had happened."""
    cfg = _cfg(chunk, left)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=44), packed_rows=False)
    lengths = [300, 260]
    utts = _utts(lengths, cfg, 11)
    Tp = subsampled_len(300)
    want = eng.streaming(2, Tp).decode(*_batch(utts, cfg.input_dim)).cpu()
    slot = eng.streaming(2, Tp, independent=True)
    plan = [(0, 0, utts[0]), (1, 0, utts[1])]
    plain = _run(eng, slot.step, 2, chunk, cfg.input_dim, plan, slot.reset)
    slot.reset()
    paused = _run(eng, slot.step, 2, chunk, cfg.input_dim, plan, slot.reset, pauses={(1, 2), (1, 3)})
    for b, n in enumerate(lengths):
        k = _out_len(n)
        assert torch.equal(paused[b], plain[b])
        assert torch.equal(paused[b][:k], want[b, :k])


def test_running_past_max_frames():
    """5. Host `valid`: the wrapper raises before anything is launched.  Device `valid`: the kernels leave the offending slot
    alone, m3_engine_stream_positions reports -1 for it, and the other slot's logits of that step and the following ones
    equal a run without the offending slot's extra step."""
    cfg = _cfg(16, 2)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=45), packed_rows=False)
    g = torch.Generator().manual_seed(12)
    win = torch.rand(6, 2, 4 * 16 + 3, cfg.input_dim, generator=g)
    slot = eng.streaming(2, 48, independent=True)                      # three chunks per stream
    full = 4 * 16 + 3
    # slot 0 live at steps 0..2 (and, offending, 3), slot 1 live at steps 2..4
    sched = [(full, 0), (full, 0), (full, full), (full, full), (0, full)]

    def run(offend, device_valid):
        slot.reset()
        outs = []
        for s, (v0, v1) in enumerate(sched):
            if s == 3 and not offend:
                v0 = 0
            valid = torch.tensor([v0, v1], dtype=torch.int32)
            lg = slot.step(win[s], valid.to(eng.device) if device_valid else valid)
            eng.stream.synchronize()
            outs.append(lg.cpu().clone())
        return outs, slot.positions().tolist()

    clean, pos = run(False, False)
    assert pos == [48, 48]
    # host valid: refused before the launch, nothing moved
    slot.reset()
    for s in range(3):
        slot.step(win[s], torch.tensor([full, 0], dtype=torch.int32))
    captures = eng.num_captures()
    with pytest.raises(M3Error, match="max_frames"):
        slot.step(win[3], torch.tensor([full, full], dtype=torch.int32))
    assert slot.positions().tolist() == [48, 0] and eng.num_captures() == captures
    # device valid: the guard is on the device
    got, pos = run(True, True)
    assert pos == [-1, 48]
    for s in (2, 3, 4):
        assert torch.equal(got[s][1], clean[s][1]), s
    for s in (0, 1, 2):
        assert torch.equal(got[s][0], clean[s][0]), s
    slot.reset(slots=[0])                                              # a restart clears the status word
    assert slot.positions().tolist() == [0, 48]


def test_decoder_in_slot_mode():
    """6. StreamingCtcDecoder over the staggered schedule, beam 10: n-best (tokens and scores) and greedy tokens of every
    stream equal the lockstep decode at B = 3; after reset(slots=[1]) a second utterance in slot 1 too."""
    chunk, left = 16, 2
    cfg = _cfg(chunk, left)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=42), packed_rows=False)
    lengths = [290, 333, 150, 230]
    utts = _utts(lengths, cfg, 9)
    Tp = subsampled_len(max(lengths))
    lock = StreamingCtcDecoder(eng.streaming(3, Tp), beam=10)
    want = lock.decode(*_batch(utts[:3], cfg.input_dim))
    want_greedy = lock.greedy()
    empty = torch.zeros(0, cfg.input_dim)
    want2 = lock.decode(*_batch([empty, utts[3], empty], cfg.input_dim))[1]
    want2_greedy = lock.greedy()[1]
    dec = StreamingCtcDecoder(eng.streaming(3, Tp, independent=True), beam=10)
    got, got_greedy = {}, {}

    def done(i, b):
        got[i] = dec.finish(slots=[b])[0]
        got_greedy[i] = dec.greedy(slots=[b])[0]
        best, gr = dec.partial(slots=[b])
        assert best[0] == got[i][0] and gr[0] == got_greedy[i]

    _run(eng, dec.step, 3, chunk, cfg.input_dim, [(0, 0, utts[0]), (1, 2, utts[1]), (2, 5, utts[2]), (1, 0, utts[3])],
         lambda slots: dec.reset(slots=slots), on_done=done)
    for i in range(3):
        assert len(want[i]) > 1 and got[i] == want[i], i
        assert got_greedy[i] == want_greedy[i] and len(want_greedy[i]) > 0, i
    assert got[3] == want2 and got_greedy[3] == want2_greedy
    assert got[3] != got[1]


def test_stream_pool():
    """7. Seven utterances through a StreamPool of B = 3 under a seeded schedule (arrival step, pieces of 1..200 frames,
    6 .. ~400 frames per utterance): every close() equals the lockstep decode at B = 3 of that utterance in the slot it
    occupied, the other slots empty.  No slot leaks."""
    chunk, left = 16, 2
    cfg = _cfg(chunk, left)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=46), packed_rows=False)
    rnd = random.Random(2024)
    lengths = [6, 400, 123, 67, 259, 31, 342]
    arrive = [0, 0, 0, 1, 2, 5, 8]                                     # more sessions than slots: the later ones wait
    utts = _utts(lengths, cfg, 13)
    Tp = subsampled_len(400)
    pool = StreamPool(StreamingCtcDecoder(eng.streaming(3, Tp, independent=True), beam=10))
    waiting, sent, sid_of, slot_of, results = list(range(7)), {}, {}, {}, {}
    step = 0
    while len(results) < 7:
        assert step < 300, "pool schedule does not end"
        while waiting and arrive[waiting[0]] <= step and pool.free_slots() > 0:
            i = waiting.pop(0)
            sid_of[i] = pool.open()
            slot_of[i] = pool.slot_of(sid_of[i])
            sent[i] = 0
        for i, sid in list(sid_of.items()):
            if i in results:
                continue
            if sent[i] < lengths[i]:
                n = min(rnd.randint(1, 200), lengths[i] - sent[i])
                pool.push(sid, utts[i][sent[i]:sent[i] + n])
                sent[i] += n
                if sent[i] == lengths[i]:
                    pool.end(sid)
        live = pool.step()
        assert set(live) <= {sid_of[i] for i in sid_of if i not in results}
        for i, sid in list(sid_of.items()):
            if i not in results and sent[i] == lengths[i] and not pool.pending(sid):
                results[i] = pool.close(sid)
        step += 1
    if len(waiting) == 0 and pool.free_slots() != 3:
        raise AssertionError("slots leaked: %s" % pool.slot_sid)
    with pytest.raises(KeyError):
        pool.push(sid_of[0], utts[0])
    lock = StreamingCtcDecoder(eng.streaming(3, Tp), beam=10)
    empty = torch.zeros(0, cfg.input_dim)
    for i in range(7):
        batch = [empty, empty, empty]
        batch[slot_of[i]] = utts[i]
        want = lock.decode(*_batch(batch, cfg.input_dim))[slot_of[i]]
        assert results[i] == want, (i, slot_of[i], results[i][:1], want[:1])
    assert results[0] == [((), 0.0)] and len(results[1]) > 1
    assert len({slot_of[i] for i in range(7)}) == 3                   # every slot was used, some of them again
    sids = [pool.open() for _ in range(3)]
    with pytest.raises(M3Error):
        pool.open()
    for sid in sids:
        pool.close(sid)
