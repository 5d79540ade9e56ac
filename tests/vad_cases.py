"""Hand-made segmenter cases shared by tests/test_vad_host.py (against the restatement) and tests/test_vad_gpu.py (against the
kernel).  The expected lists were worked out by hand from the contract of m3_vad_segments, not by running anything."""
import numpy as np

# min_silence, min_speech, pad, max_segment, split_search: small, so that every rule fires
OPTS = (6, 7, 3, 40, 16)


def _flags(n, runs):
    f = np.zeros(n, dtype=np.uint8)
    for s, e in runs:
        f[s:e] = 1
    return f


def _flat(n):
    return np.ones(n, dtype=np.float32)


def cases():
    """[(name, flags (T,) uint8, logE (T,) float32, len, expected [(start, end)])] under OPTS"""
    out = []
    # close: a gap of min_silence - 1 = 5 frames is bridged, one of min_silence = 6 is not (the padded runs then meet at 23)
    out.append(("gap5", _flags(60, [(10, 20), (25, 35)]), _flat(60), 60, [(7, 38)]))
    out.append(("gap6", _flags(60, [(10, 20), (26, 36)]), _flat(60), 60, [(7, 23), (23, 39)]))
    # close comes before open: two runs of 3 frames, 2 apart, make one of 8 >= min_speech
    out.append(("close_then_open", _flags(40, [(10, 13), (15, 18)]), _flat(40), 40, [(7, 21)]))
    # open: a run of min_speech - 1 = 6 frames is dropped, one of 7 is kept
    out.append(("speech6", _flags(40, [(10, 16)]), _flat(40), 40, []))
    out.append(("speech7", _flags(40, [(10, 17)]), _flat(40), 40, [(7, 20)]))
    # pad clipped at 0 and at len
    out.append(("pad_at_0", _flags(40, [(1, 12)]), _flat(40), 40, [(0, 15)]))
    out.append(("pad_at_len", _flags(40, [(31, 40)]), _flat(40), 40, [(28, 40)]))
    # flags behind len do not count: the row is 30 frames long
    out.append(("len_cuts_flags", _flags(40, [(20, 40)]), _flat(40), 30, [(17, 30)]))
    # split: a padded run of exactly max_segment = 40 frames is not cut, one of 41 is, at the lowest logE of [24, 40)
    out.append(("run40", _flags(50, [(3, 37)]), _flat(50), 50, [(0, 40)]))
    e = _flat(50)
    e[31] = 0.5
    e[10] = 0.0                                                    # lower, but outside the search window
    out.append(("run41", _flags(50, [(3, 38)]), e, 50, [(0, 31), (31, 41)]))
    # a tie in the window: the lowest index
    out.append(("tie", _flags(50, [(3, 38)]), _flat(50), 50, [(0, 24), (24, 41)]))
    e = _flat(50)
    e[[27, 33, 39]] = -2.0
    out.append(("tie_of_three", _flags(50, [(3, 38)]), e, 50, [(0, 27), (27, 41)]))
    # all silence, all voiced (two cuts: [24, 40) -> 30, then [54, 70) -> the first of two equal minima), len = 0
    out.append(("silence", _flags(64, []), _flat(64), 64, []))
    e = _flat(100)
    e[[30, 60, 65]] = 0.0
    out.append(("voiced", _flags(100, [(0, 100)]), e, 100, [(0, 30), (30, 60), (60, 100)]))
    out.append(("empty", _flags(16, [(0, 16)]), _flat(16), 0, []))
    return out
