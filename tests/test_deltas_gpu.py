"""Kaldi's add-deltas on the device (csrc/deltas.hip, m3asr.frontend.add_deltas / DeltaFbank) against the float64 restatement
of its contract (tests/delta_ref.py), and the streaming form against the offline one.

Bounds.  Static columns, untouched columns and zeroed rows are exact.  A delta value is one fp32 fma chain over n taps of a
table whose entries were rounded once from float64.  Against the float64 reference with float64 tables the error is at most
(n + 3) * 2^-24 * sum_j |s_j x_j|: the table entry's rounding moves every product by at most 2^-24 of itself (1 unit of the
sum in all), each of the n fmas rounds a partial sum that the sum bounds (n units), and 2 units of slack.  The reference
computes that sum per element.  Each case prints its worst err / bound before asserting (run with -s).  Everything
that is "the same frame computed elsewhere" (another batch row, the scalar against the 16-byte path, in place, a streaming
window) is torch.equal."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import delta_ref as D
from m3asr import _lib
from m3asr.frontend import (AudioWindowBuffer, DeltaFbank, Resampler, add_deltas, delta_context, num_frames)

U = 2.0 ** -24
SENTINEL = -77.25
TILE = 32                                                                       # frames per work-group (csrc/deltas.hip)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _strided(x, ld, rows_extra=2):
    """x (B, T, bins) as a row- and batch-strided device view inside a NaN buffer; 16-byte aligned iff ld % 4 == 0"""
    B, T, bins = x.shape
    buf = torch.full((B, T + rows_extra, ld), float("nan"), device="cuda")
    view = buf[:, 1:1 + T, :bins]
    view.copy_(x)
    return view


def _out(B, T, width, ld):
    buf = torch.full((B, T + 1, ld), SENTINEL, device="cuda")
    return buf, buf[:, :T, :]


def _check(got, x, n_in, lead, n_out, order, window, bins, what):
    """got (B, T_out, ld) on the host against the restatement, row by row"""
    width, worst = (order + 1) * bins, 0.0
    for b in range(x.shape[0]):
        n = min(max(n_in[b], 0), x.shape[1])
        ld_b = min(max(lead[b], 0), n)
        want_n = min(max(n_out[b], 0), n - ld_b, got.shape[1])
        y, mag = D.add_deltas(x[b, :n].numpy(), order, window, lead=ld_b, n_out=want_n)
        g = got[b].numpy()
        assert np.array_equal(g[:want_n, :bins], x[b, ld_b:ld_b + want_n].numpy()), what + ": static columns are a copy"
        assert not g[want_n:, :width].any(), what + ": frames behind n_out are zeros"
        assert np.all(g[:, width:] == SENTINEL), what + ": columns behind the row are not touched"
        for i in range(1, order + 1):
            sl = slice(i * bins, (i + 1) * bins)
            err = np.abs(g[:want_n, sl].astype(np.float64) - y[:, sl])
            bound = (2 * i * window + 1 + 3) * U * mag[:, sl]
            if want_n:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), "%s: row %d block %d err/bound %.3f" % (what, b, i, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("order,window", [(1, 2), (2, 2), (2, 3), (2, 4)])
@pytest.mark.parametrize("bins", [40, 23, 80])
def test_parity_ragged(order, window, bins):
    R, B = delta_context(order, window), 3
    width = (order + 1) * bins
    g = torch.Generator().manual_seed(100 * order + 10 * window + bins)
    worst = 0.0
    for T in sorted({1, 2, R, R + 1, 2 * R + 1, TILE + 1}):
        x = torch.randn(B, T, bins, generator=g) * 4 + 1
        n_in = [T, 0, 1] if T > 1 else [1, 0, 1]
        ld_in = bins + (4 if bins % 4 == 0 else 6)
        feat = _strided(x, ld_in)
        buf, out = _out(B, T, width, width + (8 if bins % 4 == 0 else 5))
        out_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        add_deltas(feat, _i32(n_in), order, window, out=out, out_len=out_len, bins=bins)
        torch.cuda.synchronize()
        assert out_len.cpu().tolist() == n_in
        assert torch.all(buf[:, T] == SENTINEL), "T=%d: the row behind the last is not touched" % T
        worst = max(worst, _check(out.cpu(), x, n_in, [0] * B, n_in, order, window, bins, "T=%d" % T))
        # a middle length, and n_out < n_in / > n_in
        if T > 2:
            n_in2, n_out2 = [T - 1, T, 2], [T, T - 2, 1]
            buf, out = _out(B, T, width, width + 4)
            add_deltas(feat, _i32(n_in2), order, window, out=out, n_out=_i32(n_out2), out_len=out_len, bins=bins)
            torch.cuda.synchronize()
            assert out_len.cpu().tolist() == [T - 1, T - 2, 1]
            worst = max(worst, _check(out.cpu(), x, n_in2, [0] * B, n_out2, order, window, bins, "T=%d ragged" % T))
    print("order %d window %d bins %d: worst err / bound %.3f" % (order, window, bins, worst))


@pytest.mark.parametrize("order,window", [(1, 2), (2, 2), (2, 3), (2, 4)])
@pytest.mark.parametrize("bins", [40, 23])
def test_lead(order, window, bins):
    """windows with context in front: lead = 0, R and a mixed vector; out has fewer rows than the input has frames"""
    R, B, T_in, T_out = delta_context(order, window), 3, TILE + 2 * 8 + 3, TILE + 1
    width = (order + 1) * bins
    x = torch.randn(B, T_in, bins, generator=torch.Generator().manual_seed(7 + bins + R)) * 3
    feat = _strided(x, bins + (4 if bins % 4 == 0 else 3))
    worst = 0.0
    for lead, n_in, n_out in (([0, 0, 0], [T_in, T_in, 5], [T_out, 3, 9]),
                              ([R, R, R], [T_in, R + 1, R], [T_out, 4, 2]),
                              ([0, R, 2], [T_in, T_in - 1, T_in], [T_out, T_out, T_in]),
                              ([R, T_in + 5, -3], [T_in, T_in, T_in], [T_out - R, 3, 3])):
        buf, out = _out(B, T_out, width, width + 4)
        out_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        add_deltas(feat, _i32(n_in), order, window, out=out, lead=_i32(lead), n_out=_i32(n_out), out_len=out_len, bins=bins)
        torch.cuda.synchronize()
        want_len = [min(max(o, 0), max(min(n, T_in) - min(max(l, 0), min(n, T_in)), 0), T_out) for l, n, o in zip(lead, n_in, n_out)]
        assert out_len.cpu().tolist() == want_len
        worst = max(worst, _check(out.cpu(), x, n_in, lead, n_out, order, window, bins, "lead %s" % (lead,)))
    # a frame's bits do not depend on where the window starts: a window that begins at frame 3 and has R frames of context
    whole = add_deltas(feat, _i32([T_in] * B), order, window, bins=bins)
    part = add_deltas(feat[:, 3:], _i32([T_in - 3] * B), order, window, lead=_i32([R] * B), n_out=_i32([8] * B), bins=bins)
    assert torch.equal(part[:, :8], whole[:, 3 + R:3 + R + 8]) and not part[:, 8:].any()
    print("order %d window %d bins %d: worst err / bound %.3f" % (order, window, bins, worst))


@pytest.mark.parametrize("bins", [40, 80])
def test_scalar_and_wide_paths_agree(bins):
    """the same frames through the 16-byte path (aligned, strides of whole 16 bytes) and the scalar path (odd row stride)"""
    order, window, B, T = 2, 2, 2, TILE + 5
    x = torch.randn(B, T, bins, generator=torch.Generator().manual_seed(3))
    n = _i32([T, T - 7])
    wide = add_deltas(_strided(x, bins + 4), n, order, window, bins=bins)
    odd_in = add_deltas(_strided(x, bins + 3), n, order, window, bins=bins)
    _, odd_out = _out(B, T, 3 * bins, 3 * bins + 1)
    add_deltas(_strided(x, bins + 4), n, order, window, out=odd_out, bins=bins)
    assert torch.equal(wide, odd_in) and torch.equal(wide, odd_out[..., :3 * bins])
    assert torch.all(odd_out[..., 3 * bins:] == SENTINEL)
    # ... and do not depend on the batch: row 1 alone
    alone = add_deltas(_strided(x[1:], bins + 4), n[1:].clone(), order, window, bins=bins)
    assert torch.equal(alone[0], wide[1])


@pytest.mark.parametrize("order,window,bins", [(2, 2, 40), (1, 2, 23), (2, 4, 80)])
def test_in_place(order, window, bins):
    """out is feat: the static columns are left alone (whatever they hold), the delta columns are what the two-buffer form
    writes, columns behind the row are not touched"""
    B, T, width = 3, TILE + 1, (order + 1) * bins
    ld = width + (4 if bins % 4 == 0 else 2)
    x = torch.randn(B, T, bins, generator=torch.Generator().manual_seed(5))
    n = [T, 0, 9]
    buf = torch.full((B, T, ld), SENTINEL, device="cuda")
    buf[..., :bins] = x.cuda()
    before = buf.clone()
    want = add_deltas(buf[..., :bins], _i32(n), order, window, bins=bins)
    out_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    got = add_deltas(buf, _i32(n), order, window, out=buf, out_len=out_len, bins=bins)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and out_len.cpu().tolist() == n
    assert torch.equal(buf[..., :bins], before[..., :bins]) and torch.equal(buf[..., width:], before[..., width:])
    assert torch.equal(buf[..., bins:width], want[..., bins:])
    for b in range(B):
        assert not buf[b, n[b]:, bins:width].any()
    _check(torch.cat([want[..., :width], buf[..., width:]], dim=2).cpu(), x, n, [0] * B, n, order, window, bins, "in place")


def test_bad_arguments_are_refused_and_empty_launches_nothing():
    lib = _lib.load()
    x = torch.zeros(2, 4, 8, device="cuda")
    n = _i32([4, 4])
    out = torch.zeros(2, 4, 24, device="cuda")

    def call(feat=x, order=2, window=2, bins=8, out=out, lead=None, ld_out=None, B=2, T_out=4):
        return lib.m3_add_deltas(feat.data_ptr(), feat.stride(1), feat.stride(0), feat.shape[1], n.data_ptr(),
                                 None if lead is None else lead.data_ptr(), n.data_ptr(), B, T_out, bins, order, window,
                                 out.data_ptr(), out.stride(1) if ld_out is None else ld_out, out.stride(0), None, None)

    assert call() == 0
    for kw, msg in ((dict(order=3), "order=3"), (dict(order=0), "order=0"), (dict(window=5), "window=5"), (dict(window=0), "window=0"),
                    (dict(bins=0), "bins=0"), (dict(bins=257), "bins=257"), (dict(ld_out=23), "ld_out=23"),
                    (dict(feat=out, lead=n), "in-place"), (dict(B=-1), "bad sizes")):
        assert call(**kw) != 0 and msg in _lib.last_error(), (kw, _lib.last_error())
    out.fill_(SENTINEL)
    assert call(B=0) == 0 and call(T_out=0) == 0
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    with pytest.raises(_lib.M3Error, match="order=3"):
        DeltaFbank(16, 3, 2)


# ---------------------------------------------------------------- Fbank + deltas, offline and streaming

def _speech(n, seed):
    rng = np.random.default_rng(seed)
    x = (np.cumsum(rng.normal(0, 1, n)) * 50 % 20000) - 10000 + rng.normal(0, 200, n)
    return torch.from_numpy(np.round(np.clip(x, -32768, 32767)).astype(np.int16))


@functools.lru_cache(maxsize=None)
def _dfb(bins, order, window):
    return DeltaFbank(bins, order, window, "cuda:0")


def test_delta_fbank_offline():
    """two launches: the log-Mel frames of Fbank in columns [0, bins), the deltas of exactly those frames beside them; into a
    wider buffer (an engine's input rows) as well"""
    fb = _dfb(16, 2, 2)
    pcm = torch.stack([_speech(8000, 1), _speech(8000, 2)])
    n = torch.tensor([8000, 3000])
    feat, flen = fb(pcm, n)
    static, slen = fb.fbank(pcm, n)
    assert tuple(feat.shape) == (2, 48, 48) and flen.cpu().tolist() == slen.cpu().tolist() == [48, 17]
    assert torch.equal(feat[..., :16], static)
    assert torch.equal(feat, add_deltas(static, slen, 2, 2))
    _check(torch.cat([feat, torch.full((2, 48, 1), SENTINEL, device="cuda")], 2).cpu(), static.cpu(), [48, 17], [0, 0], [48, 17], 2, 2, 16,
           "DeltaFbank")
    wide = torch.full((2, 48, 52), SENTINEL, device="cuda")
    fb(pcm, n, out=wide)
    assert torch.equal(wide[..., :48], feat) and torch.all(wide[..., 48:] == SENTINEL)
    short, slen = fb(pcm[:, :399])
    assert tuple(short.shape) == (2, 0, 48) and slen.cpu().tolist() == [0, 0]


def _emitted(frames, c):
    """frames a session assembles from `frames` feature frames: windows run while >= 7 frames remain from their start"""
    n = 0
    while D.next_window_valid(frames, n + 1, c, True):
        n += 1
    return 4 * c * n + D.next_window_valid(frames, n, c, True)


def _stream(buf, fb, x, pieces, c, resampler=None):
    """push x through the window buffer in pieces; featurise every window with the streaming form -> the frames a session
    assembles: the first 4 c frames of every window, all of the last"""
    R, rows, sent, i = fb.context, [], 0, 0
    out = torch.zeros(1, 4 * c + 3, fb.width + 4, device="cuda")
    while sent < x.shape[0] or not buf.drained():
        if sent < x.shape[0]:
            k = min(pieces[i % len(pieces)], x.shape[0] - sent)
            buf.push(x[sent:sent + k])
            sent, i = sent + k, i + 1
            if sent == x.shape[0]:
                buf.end()
        while buf.ready():
            v = buf.ready()
            if resampler is None:
                win, real = buf.take()
                pcm, n = win.unsqueeze(0), torch.tensor([real])
            else:
                win, in0, n_in, out0, n_out = buf.take()
                span = torch.zeros(1, -(-win.numel() // 8) * 8, dtype=torch.int16, device="cuda")
                span[0, :win.numel()] = win.reshape(-1).cuda()
                pcm = torch.zeros(1, buf.window, device="cuda")
                resampler.launch(span, torch.tensor([in0], device="cuda"), _i32([n_in]), torch.tensor([out0], device="cuda"),
                                 _i32([n_out]), pcm)
                n = torch.tensor([n_out])
            out.fill_(SENTINEL)
            _, got_len = fb(pcm, n, out=out, lead=torch.tensor([buf.lead]), n_out=torch.tensor([v]))
            assert got_len.cpu().tolist() == [v] and torch.all(out[..., fb.width:] == SENTINEL) and not out[0, v:, :fb.width].any()
            last = buf.drained()
            rows.append(out[0, :v if last else 4 * c, :fb.width].clone())
    return torch.cat(rows)


@pytest.mark.parametrize("c,order,window", [(1, 2, 2), (4, 2, 2), (1, 2, 3)])
def test_streaming_equals_offline(c, order, window):
    """1 s pushed in odd pieces through AudioWindowBuffer(context=R) + DeltaFbank(lead=): the assembled frames are the offline
    DeltaFbank's, bit for bit -- also with R = 6 > 4 c = 4, where the second window's lead is short of R"""
    fb = _dfb(16, order, window)
    x = _speech(16000, 11)
    want = fb(x)[0][0]
    got = _stream(AudioWindowBuffer(c, context=fb.context), fb, x, [1, 161, 1601, 4000, 333], c)
    assert want.shape[0] == 98 and got.shape[0] == _emitted(98, c) >= 95 and torch.equal(got, want[:got.shape[0]])


def test_streaming_equals_offline_at_8k():
    fb, rs = _dfb(16, 2, 2), Resampler(8000, "cuda:0")
    x = _speech(8000, 12)
    want = fb(*rs(x.unsqueeze(0)))[0][0]
    got = _stream(AudioWindowBuffer(1, sample_rate=8000, context=fb.context), fb, x.unsqueeze(1), [77, 801, 2000], 1, resampler=rs)
    assert want.shape[0] == 98 and got.shape[0] == _emitted(98, 1) == 95 and torch.equal(got, want[:95])
