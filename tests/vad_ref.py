"""Float64 restatement of the long-form contracts of include/m3asr.h (m3_vad_log_energy, m3_vad_decide, m3_vad_segments,
m3_segment_gather) and of LongFormTranscriber.plan_batches' invariants.  Written from the contracts, frame by
frame and run by run, with none of the product's structure (no masks, no streaming, no tiles).  numpy only."""
import numpy as np

FRAME, SHIFT = 400, 160
FLT_EPSILON = float(np.finfo(np.float32).eps)


def num_frames(n):
    return 0 if n < FRAME else 1 + (n - FRAME) // SHIFT


def log_energy(x, T=None):
    """x: the samples of one row (any real dtype) -> (T,) float64: log(max(sum (x - mean)^2, FLT_EPSILON)) of every frame,
    zeros behind the last, and the frame count min(num_frames(len(x)), T)"""
    x = np.asarray(x, dtype=np.float64)
    n = num_frames(len(x))
    T = n if T is None else T
    n = min(n, T)
    out = np.zeros(T)
    for k in range(n):
        f = x[SHIFT * k: SHIFT * k + FRAME]
        out[k] = np.log(max(float(((f - f.mean()) ** 2).sum()), FLT_EPSILON))
    return out, n


def threshold(logE, n, energy_threshold, mean_scale):
    mean = float(np.asarray(logE[:n], dtype=np.float64).mean()) if n > 0 else 0.0
    return np.float32(float(energy_threshold) + float(mean_scale) * mean)


def decide(logE, n, energy_threshold=5.0, mean_scale=0.5, context=0, proportion=0.6):
    """logE (T,) float32 values, n valid frames -> ((T,) uint8 flags, float32 threshold).  The comparison num >= den *
    proportion is made in float32, as Kaldi makes it."""
    logE = np.asarray(logE)
    thr = threshold(logE, n, energy_threshold, mean_scale)
    flags = np.zeros(len(logE), dtype=np.uint8)
    for t in range(n):
        lo, hi = max(t - context, 0), min(t + context, n - 1)
        den = hi - lo + 1
        num = int(sum(1 for u in range(lo, hi + 1) if np.float32(logE[u]) > thr))
        flags[t] = 1 if np.float32(num) >= np.float32(den) * np.float32(proportion) else 0
    return flags, thr


def margin(logE, n, energy_threshold, mean_scale):
    """distance of the closest valid log-energy to the threshold (inf for an empty row)"""
    if n == 0:
        return float("inf")
    thr = float(threshold(logE, n, energy_threshold, mean_scale))
    return float(np.abs(np.asarray(logE[:n], dtype=np.float64) - thr).min())


def options_ok(min_silence, min_speech, pad, max_segment, split_search):
    return min_silence >= 0 and pad >= 0 and min_speech >= 7 and 2 * pad <= min_silence and 1 <= split_search <= max_segment - 7


def _runs(v):
    """[start, end) of every maximal run of true values"""
    out, s = [], None
    for t, on in enumerate(list(v) + [False]):
        if on and s is None:
            s = t
        elif not on and s is not None:
            out.append([s, t])
            s = None
    return out


def segments(flags, logE, n, min_silence, min_speech, pad, max_segment, split_search):
    """close, open, pad, split -- in that order -> [(start, end)] in ascending order"""
    assert options_ok(min_silence, min_speech, pad, max_segment, split_search)
    v = [bool(f) for f in np.asarray(flags)[:n]]
    runs = _runs(v)
    for (_, e0), (s1, _) in zip(runs[:-1], runs[1:]):             # close: a silence run strictly between two voiced runs
        if s1 - e0 < min_silence:
            for t in range(e0, s1):
                v[t] = True
    runs = [r for r in _runs(v) if r[1] - r[0] >= min_speech]     # open
    runs = [[max(s - pad, 0), min(e + pad, n)] for s, e in runs]  # pad
    assert all(a[1] <= b[0] for a, b in zip(runs[:-1], runs[1:])), "padded runs overlap"    # they may meet: 2 pad == min_silence
    out = []
    for s, e in runs:                                             # split
        while e - s > max_segment:
            lo, hi = s + max_segment - split_search, s + max_segment
            cut = lo + int(np.argmin(np.asarray(logE[lo:hi], dtype=np.float64)))      # the first of equal minima
            out.append((s, cut))
            s = cut
        out.append((s, e))
    return out


def gather(src, jobs, T_max, dst):
    """src (T_all, >= cols), jobs [(src_row, start, end)], dst (B, T_max, cols) is written in place -> lengths"""
    lens = []
    for b, (r, s, e) in enumerate(jobs):
        n = min(e - s, T_max)
        dst[b, :n] = src[r + s: r + s + n, :dst.shape[2]]
        dst[b, n:] = 0
        lens.append(n)
    return lens


def check_plan(segs, plan, max_batch, max_batch_frames, bucket):
    """the invariants of plan_batches: every segment exactly once; both caps; T_max on the bucket grid and the smallest that
    holds the batch; segments in descending length across the plan"""
    seen = [i for idx, _ in plan for i in idx]
    assert sorted(seen) == list(range(len(segs))), "every segment exactly once"
    lengths = [segs[i][1] - segs[i][0] for i in seen]
    assert lengths == sorted(lengths, reverse=True), "longest first"
    for idx, T_max in plan:
        longest = max(segs[i][1] - segs[i][0] for i in idx)
        assert 1 <= len(idx) <= max_batch and len(idx) * T_max <= max_batch_frames
        assert T_max % bucket == 0 and longest <= T_max < longest + bucket
