"""Host restatement of the blank-frame skipping contract of include/m3asr.h ("m3_wfst_skip"), in plain numpy.

select() is the rule, frame by frame, over a state that carries from call to call; RefSkipSearch is select() in front of
wfst_ref.RefSearch plus the frame map, i.e. what m3asr.wfst.CtcWfstSearch(blank_skip=p) computes.  The device must equal both
exactly: the emitted rows bit for bit, the counts, the map, the saved row, and through the search words, mapped frames, cost
bits, reached_final and status.
"""
import numpy as np

import wfst_ref as R

F = np.float32


def log_thresh(p):
    """the threshold CtcWfstSearch(blank_skip=p) hands to the library"""
    return F(np.log(p))


class SkipState:
    """One utterance's state: the header's five numbers, the saved row and the map (unbounded here; the device stores its
    first max_frames entries).  reinserted counts how often the rule put a saved row back."""

    def __init__(self, blank):
        self.blank = int(blank)
        self.reset()

    def reset(self):
        self.last_blank, self.last_best, self.saved_frame, self.n_seen, self.n_kept = 0, self.blank, 0, 0, 0
        self.saved, self.map, self.reinserted = None, [], 0
        return self


def argmax(row):
    """the smallest index of the row's maximum, a NaN entry counting as -inf"""
    return int(np.argmax(np.where(np.isnan(row), F(-np.inf), row)))


def select(logp, blank, log_thresh, state, reinsert=True):
    """logp (n, V) float32 rows of one utterance -> the emitted rows (k, V), k <= n + 1.  reinsert=False drops the rule's
    re-insertion (what a naive skipper does; only to show that the tests' cases need it)."""
    logp = np.asarray(logp, dtype=np.float32)
    out = []

    def emit(row, frame):
        out.append(row)
        state.map.append(frame)
        state.n_kept += 1

    for row in logp:
        t = state.n_seen
        state.n_seen += 1
        if row[blank] > F(log_thresh):
            state.last_blank, state.saved, state.saved_frame = 1, row.copy(), t
            continue
        best = argmax(row)
        if reinsert and best != blank and state.last_blank and best == state.last_best:
            emit(state.saved, state.saved_frame)
            state.reinserted += 1
        emit(row, t)
        state.last_best, state.last_blank = best, 0
    return np.stack(out) if out else np.zeros((0, logp.shape[1]), dtype=np.float32)


def map_frames(frames, state, max_frames=None):
    held = state.n_kept if max_frames is None else min(state.n_kept, int(max_frames))
    return [state.map[r] if 0 <= r < held else state.n_seen for r in frames]


class RefSkipSearch:
    """select + wfst_ref.RefSearch + the frame map.  max_frames bounds the decoded frames (the search's) and the map."""

    def __init__(self, g, beam, max_active, blank_skip, blank=0, acoustic_scale=1.0, max_frames=None, reinsert=True, **caps):
        self.search = R.RefSearch(g, beam, max_active, acoustic_scale, max_frames=max_frames, **caps)
        self.state, self.blank, self.thresh, self.max_frames, self.reinsert = SkipState(blank), int(blank), log_thresh(blank_skip), max_frames, reinsert

    def reset(self):
        self.search.reset()
        self.state.reset()
        return self

    def advance(self, logp):
        self.search.advance(select(logp, self.blank, self.thresh, self.state, self.reinsert))
        return self

    def result(self, final=True):
        r = self.search.result(final)
        r["frames"] = map_frames(r["frames"], self.state, self.max_frames)
        return r

    def frames(self):
        return self.state.n_seen, self.state.n_kept
