"""Float64 restatement of Kaldi's DeltaFeatures (feat/feature-functions.cc: DeltaFeatures::DeltaFeatures and ::Process, what
add-deltas and the loader's compute_deltas run) -- the contract of m3_add_deltas (include/m3asr.h), test-side only.

It is written the way Kaldi computes it: ONE composite filter per block, scales_i = conv(scales_{i-1}, [-W..W]) / sum j^2,
applied to the STATIC frames with the frame index clamped to the utterance.  `iterated_replicate` is the other reading -- a
first-order delta applied `order` times, each time with replicate padding -- which is what torchaudio.functional.compute_deltas
does; it differs from Kaldi in the first and last `window` frames of the delta-delta block and is here only so that a test
can show that this restatement is not that one.

`window_rule` / `session_windows` restate, by brute force, which delta frames a stream's window n produces and which static
frames it carries for them."""
import numpy as np


def scales(order, window):
    """[scales_0, ..., scales_order] in float64; scales_i has 2 i window + 1 taps for offsets -i window .. i window."""
    out = [np.array([1.0])]
    norm = float(sum(j * j for j in range(-window, window + 1)))
    for i in range(1, order + 1):
        prev = out[-1]
        cur = np.zeros(prev.shape[0] + 2 * window)
        for k in range(prev.shape[0]):
            for j in range(-window, window + 1):
                cur[k + j + window] += j * prev[k] / norm
        out.append(cur)
    return out


def add_deltas(x, order, window, lead=0, n_out=None, tables=None):
    """x (n, bins) static frames of one row -> (y (n_out, (order + 1) * bins) float64, mag (same shape) = sum_j |s_j x_j| per
    element (1 * |x| in the static block).  Output frame t is centred on input frame lead + t, taps clamped to [0, n - 1].
    tables: the filters to use (default: scales(order, window) in float64)."""
    x = np.asarray(x, dtype=np.float64)
    n, bins = x.shape
    n_out = max(n - lead, 0) if n_out is None else min(n_out, max(n - lead, 0))
    tabs = scales(order, window) if tables is None else [np.asarray(t, dtype=np.float64) for t in tables]
    y = np.zeros((n_out, (order + 1) * bins))
    mag = np.zeros_like(y)
    for t in range(n_out):
        for i in range(order + 1):
            for k, s in enumerate(tabs[i]):
                j = k - i * window
                src = x[min(max(lead + t + j, 0), n - 1)]
                y[t, i * bins:(i + 1) * bins] += s * src
                mag[t, i * bins:(i + 1) * bins] += np.abs(s * src)
    return y, mag


def iterated_replicate(x, order, window):
    """NOT the contract: the first-order delta applied `order` times with replicate padding each time."""
    x = np.asarray(x, dtype=np.float64)
    s1 = scales(1, window)[1]
    blocks = [x]
    for _ in range(order):
        prev = blocks[-1]
        pad = np.concatenate([np.repeat(prev[:1], window, 0), prev, np.repeat(prev[-1:], window, 0)])
        blocks.append(sum(s1[k] * pad[k:k + prev.shape[0]] for k in range(2 * window + 1)))
    return np.concatenate(blocks, axis=1)


def next_window_valid(buffered, chunks_done, c, ended):
    """serve.next_window_valid, restated: a window runs when it is full, or the stream has ended and >= 7 frames remain."""
    left = buffered - 4 * c * chunks_done
    if left >= 4 * c + 3:
        return 4 * c + 3
    return left if ended and left >= 7 else 0


def window_rule(frames, n, c, R, ended):
    """Window n of a segment of which `frames` static frames exist: None when it cannot run, else (s0, s1, lead, v): it
    produces delta frames [4 c n, 4 c n + v) from static frames [s0, s1), the first `lead` of which are context only."""
    usable = frames if ended else max(frames - R, 0)
    v = next_window_valid(usable, n, c, ended)
    if v == 0:
        return None
    s0 = max(4 * c * n - R, 0)
    s1 = min(4 * c * n + v + R, frames)
    return s0, s1, 4 * c * n - s0, v
