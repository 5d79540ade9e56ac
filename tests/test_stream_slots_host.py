"""Host-only parts of slot-mode streaming (m3asr/serve.py): the window rule against the slices StreamingEncoder.decode cuts,
and StreamPool's slot accounting with a stub decoder.  No GPU, no engine."""
import random

import pytest
import torch

from m3asr._lib import M3Error
from m3asr.serve import StreamPool, WindowBuffer, next_window_valid


def _decode_windows(feat, c):
    """The windows and `valid` values StreamingEncoder.decode hands to step() for ONE utterance (engine.py, decode): window n =
    frames [4 c n, 4 c n + 4 c + 3) of the zero-padded utterance, valid = clamp(len - 4 c n, 0, 4 c + 3), below 7 -> 0."""
    T, window = int(feat.shape[0]), 4 * c + 3
    Tp = ((T - 1) // 2 - 1) // 2 if T >= 7 else 0
    n_chunks = -(-Tp // c)
    padded = torch.zeros(max(T, 4 * c * n_chunks + 3) + window, feat.shape[1])
    padded[:T] = feat
    out = []
    for n in range(n_chunks):
        left = min(max(T - 4 * c * n, 0), window)
        left = left if left >= 7 else 0
        if left:
            w = padded[4 * c * n: 4 * c * n + window].clone()
            w[left:] = 0
            out.append((w, left))
    return out


@pytest.mark.parametrize("c", [4, 16])
def test_window_buffer_cuts_what_decode_cuts(c):
    rnd = random.Random(5)
    g = torch.Generator().manual_seed(1)
    lengths = list(range(0, 8)) + [4 * c + 2, 4 * c + 3, 4 * c + 4, 8 * c + 2, 8 * c + 3, 8 * c + 10, 333, 517]
    for T in lengths:
        feat = torch.rand(T, 5, generator=g)
        want = _decode_windows(feat, c)
        for trial in range(3):
            wb, got, sent = WindowBuffer(c, 5), [], 0
            while sent < T:
                n = min(rnd.randint(1, 1 if trial == 0 else 200), T - sent)
                wb.push(feat[sent:sent + n])
                sent += n
                while wb.ready():                       # before the end only FULL windows may run
                    w, v = wb.take()
                    assert v == 4 * c + 3
                    got.append((w.clone(), v))
            assert not wb.drained()
            wb.end()
            while wb.ready():
                w, v = wb.take()
                got.append((w.clone(), v))
            assert wb.drained()
            assert [v for _, v in got] == [v for _, v in want], (T, trial)
            for (w, _), (x, _) in zip(got, want):
                assert torch.equal(w, x), (T, trial)
            assert wb.buf.shape[0] <= 4 * c + 3 + 200    # consumed frames are dropped
            with pytest.raises(ValueError):
                wb.push(feat[:1])


def test_next_window_valid_rule():
    c, w = 16, 67
    assert next_window_valid(66, 0, c, False) == 0 and next_window_valid(67, 0, c, False) == w
    assert next_window_valid(66, 0, c, True) == 66 and next_window_valid(6, 0, c, True) == 0 and next_window_valid(7, 0, c, True) == 7
    assert next_window_valid(67, 1, c, True) == 0            # the 3 overlap frames alone give no output
    assert next_window_valid(64 + 7, 1, c, True) == 7 and next_window_valid(64 + 67, 1, c, False) == w
    assert next_window_valid(1000, 3, c, True) == w


class _StubDecoder:
    """What StreamPool needs of a decoder, recording the calls."""

    def __init__(self):
        self.steps, self.resets, self.frames = [], [], {}

    def reset(self, slots=None):
        self.resets.append(list(slots))
        for b in slots:
            self.frames[b] = 0

    def step(self, window, valid):
        self.steps.append((window.clone(), valid.clone()))
        for b, v in enumerate(valid.tolist()):
            self.frames[b] = self.frames.get(b, 0) + v

    def partial(self, slots=None):
        return [((b,), float(self.frames[b])) for b in slots], [[self.frames[b]] for b in slots]

    def finish(self, slots=None):
        return [[((b,), float(self.frames[b]))] for b in slots]


def test_stream_pool_slot_accounting():
    c, idim, B = 4, 3, 3
    dec = _StubDecoder()
    pool = StreamPool(dec, B=B, chunk=c, input_dim=idim)
    window = 4 * c + 3
    a, b_, c_ = pool.open(), pool.open(), pool.open()
    assert [pool.slot_of(s) for s in (a, b_, c_)] == [0, 1, 2] and dec.resets == [[0], [1], [2]]
    with pytest.raises(M3Error):
        pool.open()
    assert pool.step() == [] and dec.steps == []                       # nothing buffered: no engine call at all
    fa = torch.arange(window * idim, dtype=torch.float32).view(window, idim)
    pool.push(a, fa)                                                   # a: exactly one full window
    pool.push(b_, torch.ones(window - 1, idim))                        # b: one frame short
    pool.push(c_, torch.ones(9, idim))                                 # c: 9 frames, then ended -> a final short window
    pool.end(c_)
    assert pool.pending(a) and not pool.pending(b_) and pool.pending(c_)
    assert sorted(pool.step()) == sorted([a, c_])
    win, valid = dec.steps[-1]
    assert valid.tolist() == [window, 0, 9]
    assert torch.equal(win[0], fa) and torch.equal(win[2, :9], torch.ones(9, idim)) and float(win[2, 9:].abs().max()) == 0
    assert pool.step() == [] and len(dec.steps) == 1                   # a has 3 overlap frames left, b still short
    pool.push(b_, torch.ones(1, idim))
    assert pool.step() == [b_] and dec.steps[-1][1].tolist() == [0, window, 0]
    best, greedy = pool.partial(c_)
    assert best == ((2,), 9.0) and greedy == [9]
    assert pool.close(c_) == [((2,), 9.0)] and pool.free_slots() == 1
    with pytest.raises(KeyError):
        pool.push(c_, torch.ones(1, idim))
    d = pool.open()                                                    # the freed slot is taken again, and restarted
    assert pool.slot_of(d) == 2 and dec.resets[-1] == [2] and dec.frames[2] == 0
    pool.end(a)
    assert not pool.pending(a)                                         # 3 frames left: no output frame fits
    pool.push(d, torch.ones(4 * c + window, idim))     # d: two full windows at once -> one per step
    assert pool.step() == [d] and pool.step() == [d] and pool.step() == []
    for s in (a, b_, d):
        pool.close(s)
    assert pool.free_slots() == B and [pool.open() for _ in range(B)] and pool.free_slots() == 0
