"""Float64 restatement of the resampler's contract (include/m3asr.h, the m3_resample block), written from the
text of the contract and not from the library: Kaldi's LinearResample as ResampleWaveform calls it, cutoff
0.99 * 0.5 * min(ri, ro), 6 zeros, with the two departures (ri == ro is the identity; channels are reduced on the way in).

    tables(ri, ro)                         -> Tables(first, n, w [per phase float64], in_unit, out_unit, ...)
    num_samples(ri, ro, n, flush)          -> outputs that n input samples admit
    input_span(ri, ro, out0, n_out)        -> [first_in, end_in) of absolute input indices
    downmix(x (N, C), channel)             -> mono, float32 arithmetic in channel order (it is part of the input, exact)
    resample(x, ri, ro, in0, out0, n_out)  -> (y float64, bound float64): y[i] = output out0 + i from the mono samples x that
                                              stand at absolute indices in0 .., zeros elsewhere; bound[i] = sum_j |w_j x_j|
    resample32(x, weights32, ...)          -> the same sum done with np.float32 scalars in the kernel's order (one accumulator
                                              from 0, ascending j, multiply then add) on a table of float32 weights
"""
import collections
import math

import numpy as np

Z = 6
Tables = collections.namedtuple("Tables", "first n w in_unit out_unit max_taps floats")


def _rates(ri, ro):
    g = math.gcd(ri, ro)
    cutoff = 0.99 * 0.5 * min(ri, ro)
    return ri // g, ro // g, cutoff, Z / (2 * cutoff)


def _phase(ri, ro, p):
    """(first, n) of phase p"""
    if ri == ro:
        return 0, 1
    _, _, _, ww = _rates(ri, ro)
    t = p / ro
    first = math.ceil((t - ww) * ri)
    return first, math.floor((t + ww) * ri) - first + 1


def _weight(ri, cutoff, ww, dt):
    window = 0.5 * (1 + math.cos(2 * math.pi * cutoff / Z * dt)) if abs(dt) < ww else 0.0
    filt = math.sin(2 * math.pi * cutoff * dt) / (math.pi * dt) if dt != 0 else 2 * cutoff
    return window * filt / ri


def table_shape(ri, ro):
    """(phases, max_taps, sum of taps) without the weights: cheap for any pair"""
    in_unit, out_unit, _, _ = _rates(ri, ro)
    n = [_phase(ri, ro, p)[1] for p in range(out_unit)]
    return out_unit, max(n), sum(n)


def tables(ri, ro):
    in_unit, out_unit, cutoff, ww = _rates(ri, ro)
    first, n, w = [], [], []
    for p in range(out_unit):
        f, k = _phase(ri, ro, p)
        first.append(f)
        n.append(k)
        if ri == ro:
            w.append(np.ones(1))
        else:
            t = p / ro
            w.append(np.array([_weight(ri, cutoff, ww, (f + j) / ri - t) for j in range(k)], dtype=np.float64))
    return Tables(np.array(first, np.int64), np.array(n, np.int64), w, in_unit, out_unit, max(n), sum(n))


def num_samples(ri, ro, n, flush=True):
    if n <= 0:
        return 0
    if ri == ro:
        return n
    _, _, _, ww = _rates(ri, ro)
    tick = ri * ro // math.gcd(ri, ro)
    L = n * (tick // ri)
    if not flush:
        L -= math.floor(ww * tick)
    if L <= 0:
        return 0
    last = L // (tick // ro)
    if last * (tick // ro) == L:
        last -= 1
    return last + 1


def input_span(ri, ro, out0, n_out):
    in_unit, out_unit, _, _ = _rates(ri, ro)
    f, _ = _phase(ri, ro, out0 % out_unit)
    lo = f + (out0 // out_unit) * in_unit
    if n_out <= 0:
        return lo, lo
    last = out0 + n_out - 1
    f, k = _phase(ri, ro, last % out_unit)
    return lo, f + (last // out_unit) * in_unit + k


def downmix(x, channel=-1):
    """x (N, C) int16 / float32 -> mono float32: the mean of all channels summed in channel order with a true division, or
    one channel.  Every step is a float32 operation with one correctly rounded answer, so this is the kernel's input."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    x = x.astype(np.float32)
    if channel >= 0:
        return x[:, channel].copy()
    acc = np.zeros(x.shape[0], np.float32)
    for c in range(x.shape[1]):
        acc = acc + x[:, c]
    return acc / np.float32(x.shape[1])


def _taps(tab, o):
    p, u = o % tab.out_unit, o // tab.out_unit
    return p, int(tab.first[p]) + u * tab.in_unit


def resample(x, ri, ro, in0=0, out0=0, n_out=None, tab=None):
    """x: the mono samples standing at absolute input indices [in0, in0 + len(x)); zeros elsewhere."""
    tab = tab if tab is not None else tables(ri, ro)
    x = np.asarray(x, dtype=np.float64)
    if n_out is None:
        n_out = num_samples(ri, ro, len(x), True)
    y, bound = np.zeros(n_out), np.zeros(n_out)
    for i in range(n_out):
        p, s = _taps(tab, out0 + i)
        w = tab.w[p]
        lo = s - in0
        a, b = max(lo, 0), min(lo + len(w), len(x))
        if a < b:
            prod = w[a - lo:b - lo] * x[a:b]
            y[i], bound[i] = prod.sum(), np.abs(prod).sum()
    return y, bound


def resample32(x, first, n, weights, in_unit, out_unit, in0=0, out0=0, n_out=0):
    """The kernel's arithmetic on the library's table: first / n (out_unit,), weights (out_unit, max_taps) float32."""
    x = np.asarray(x, dtype=np.float32)
    y = np.zeros(n_out, np.float32)
    for i in range(n_out):
        o = out0 + i
        p, u = o % out_unit, o // out_unit
        lo = int(first[p]) + u * in_unit - in0
        acc = np.float32(0)
        for j in range(int(n[p])):
            k = lo + j
            if 0 <= k < len(x):
                acc = np.float32(acc + np.float32(weights[p, j] * x[k]))
        y[i] = acc
    return y
