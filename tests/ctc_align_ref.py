"""Restatement of the CTC forced-alignment contract (include/m3asr.h, m3_ctc_align_*) in numpy.  Test-side only.

    e[t][v]   log-probabilities of T frames,  y[0..L) tokens in [0, V) other than `blank`
    S = 2 L + 1 states, lab(s) = blank for even s, y[s >> 1] for odd s
    a[0][0] = e[0][blank], a[0][1] = e[0][y[0]], all other states -inf
    a[t][s] = best + e[t][lab(s)], best over stay a[t-1][s], step a[t-1][s-1] (s >= 1), skip a[t-1][s-2] (s odd, s >= 3,
              lab(s) != lab(s-2)); a later move replaces an earlier one only when strictly greater
    final state S - 1, unless S > 1 and a[T-1][S-2] > a[T-1][S-1]; the recorded moves lead back from it

`dtype` is the arithmetic: numpy.float32 is what the device computes bit for bit (one add on one maximum per cell, nothing to
reassociate), numpy.float64 the yardstick.  A frame is reduced with whole-array operations, which changes no value: maxima and
one addition per cell.
"""
import collections

import numpy as np

OK, NO_ALIGNMENT, BAD_INPUT = 0, 1, 2

# state: (T,) int32, -1 everywhere unless status == OK; start / end / peak: (L,) int32; peak_logp: (L,) dtype
Aligned = collections.namedtuple("Aligned", "status score state start end peak peak_logp")


def _failed(code, T, L, dtype):
    return Aligned(code, dtype(-np.inf), np.full(T, -1, np.int32), np.full(L, -1, np.int32), np.full(L, -1, np.int32),
                   np.full(L, -1, np.int32), np.full(L, -np.inf, dtype))


def repeats(y):
    return sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])


def align_emit_ref(emit, y, dtype=np.float32):
    """The path stage on the L + 1 emission columns the trellis reads: emit (T, >= L + 1), column 0 the blank's log-probability,
    column 1 + i that of y[i].  The tokens are taken as valid (they only tell which neighbours are equal)."""
    y = [int(v) for v in y]
    L, T = len(y), int(emit.shape[0])
    emit = np.asarray(emit, dtype=dtype)
    if T == 0:
        return Aligned(OK, dtype(0), np.zeros(0, np.int32), *(np.zeros(0, np.int32),) * 3, np.zeros(0, dtype)) if L == 0 \
            else _failed(NO_ALIGNMENT, T, L, dtype)
    if T < L + repeats(y):
        return _failed(NO_ALIGNMENT, T, L, dtype)
    S = 2 * L + 1
    col = np.array([1 + (s >> 1) if s & 1 else 0 for s in range(S)])
    skip_ok = np.array([bool(s & 1) and s >= 3 and y[s >> 1] != y[(s >> 1) - 1] for s in range(S)])
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype=dtype)
    a[0] = emit[0, 0]
    if L > 0:
        a[1] = emit[0, 1]
    moves = np.zeros((T, S), np.int8)
    for t in range(1, T):
        step = np.concatenate([[ninf], a[:-1]]).astype(dtype)
        skip = np.where(skip_ok, np.concatenate([[ninf, ninf], a[:-2]])[:S], ninf).astype(dtype)
        best, mv = a.copy(), np.zeros(S, np.int8)
        m = step > best
        best[m], mv[m] = step[m], 1
        m = skip > best
        best[m], mv[m] = skip[m], 2
        a = (best + emit[t, col]).astype(dtype)
        moves[t] = mv
    final = S - 2 if S > 1 and a[S - 2] > a[S - 1] else S - 1
    score = a[final]
    if score == ninf:
        return _failed(NO_ALIGNMENT, T, L, dtype)
    state = np.zeros(T, np.int32)
    s = final
    for t in range(T - 1, 0, -1):
        state[t] = s
        s -= int(moves[t, s])
    state[0] = s
    start, end, peak = (np.full(L, -1, np.int32) for _ in range(3))
    logp = np.full(L, ninf, dtype=dtype)
    for i in range(L):
        frames = np.nonzero(state == 2 * i + 1)[0]
        if len(frames) == 0:           # unreachable for a finite score; kept so that a broken input cannot raise here
            continue
        start[i], end[i] = frames[0], frames[-1] + 1
        seg = emit[start[i]:end[i], 1 + i]
        peak[i] = start[i] + int(np.argmax(seg))       # argmax: the first of equal maxima
        logp[i] = seg[peak[i] - start[i]]
    return Aligned(OK, dtype(score), state, start, end, peak, logp)


def ctc_align_ref(e, y, blank=0, dtype=np.float32):
    """e (T, V) log-probabilities, y tokens -> Aligned.  A token that is `blank` or outside [0, V): BAD_INPUT."""
    e = np.asarray(e)
    T, V = int(e.shape[0]), int(e.shape[1])
    y = [int(v) for v in y]
    if any(v == blank or not 0 <= v < V for v in y):
        return _failed(BAD_INPUT, T, len(y), dtype)
    return align_emit_ref(e[:, [blank] + y], y, dtype)


def log_softmax_ref(x, dtype=np.float32):
    """Row-wise log-softmax in `dtype` the way the emit stage takes it: maximum subtracted, then one logarithm of the sum."""
    x = np.asarray(x, dtype=dtype)
    mx = x.max(axis=-1, keepdims=True)
    lse = mx + np.log(np.exp(x - mx).sum(axis=-1, keepdims=True, dtype=dtype)).astype(dtype)
    return (x - lse).astype(dtype)


def collapse(labels, blank=0):
    """CTC's many-to-one map of a frame labelling: drop repeats, then blanks."""
    out, prev = [], None
    for v in labels:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out


def path_labels(state, y, blank=0):
    return [blank if s % 2 == 0 else int(y[s >> 1]) for s in state]


def is_valid_path(state, y):
    """state is a monotone walk over the trellis of y: starts in 0 / 1, ends in S - 1 / S - 2, moves by 0, 1 or an allowed 2."""
    S, T = 2 * len(y) + 1, len(state)
    if T == 0:
        return len(y) == 0
    if state[0] not in (0, 1)[:S] or state[-1] not in ((S - 1, S - 2) if S > 1 else (0,)):
        return False
    for t in range(1, T):
        d, s = state[t] - state[t - 1], state[t]
        if d not in (0, 1, 2) or not 0 <= s < S:
            return False
        if d == 2 and not (s & 1 and s >= 3 and y[s >> 1] != y[(s >> 1) - 1]):
            return False
    return True


def brute_force(e, y, blank=0):
    """max over all V^T frame labellings that collapse to y of the float64 sum of their log-probabilities; -inf if none"""
    import itertools
    e = np.asarray(e, dtype=np.float64)
    T, V = e.shape
    best = -np.inf
    for lab in itertools.product(range(V), repeat=T):
        if collapse(lab, blank) == list(y):
            best = max(best, float(sum(e[t, v] for t, v in enumerate(lab))))
    return best
