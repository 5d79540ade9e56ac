"""The endpoint rule of m3_ctc_endpoint_* (include/m3asr.h) in plain Python, one frame at a time: the yardstick
of tests/test_ctc_endpoint_gpu.py.  Nothing here is clever on purpose."""
import numpy as np

FRESH = (0, 0, 0, -1, -1, 0, -1)      # frames, trailing_blank, decoded, first_speech, last_speech, fired_rule, fired_frame


class EndpointRef:
    """One stream.  rules: [(must_decoded, min_trailing frames, min_length frames)]; log_thr: the float32 threshold."""

    def __init__(self, blank, log_thr, rules):
        self.blank, self.log_thr, self.rules = int(blank), np.float32(log_thr), [tuple(int(v) for v in r) for r in rules]
        self.reset()

    def reset(self):
        self.frames, self.trailing_blank, self.decoded, self.first_speech, self.last_speech, self.fired_rule, self.fired_frame = FRESH

    def frame(self, top_logp0, top_idx0):
        """One real frame: entry 0 of its top-k."""
        if self.fired_rule:
            return
        self.frames += 1
        if int(top_idx0) == self.blank and np.float32(top_logp0) > self.log_thr:
            self.trailing_blank += 1
        else:
            self.trailing_blank = 0
        if int(top_idx0) != self.blank:
            self.decoded = 1
            self.last_speech = self.frames - 1
            if self.first_speech == -1:
                self.first_speech = self.frames - 1
        for r, (must_decoded, min_trailing, min_length) in enumerate(self.rules, 1):
            if (self.decoded or not must_decoded) and self.trailing_blank >= min_trailing and self.frames >= min_length:
                self.fired_rule, self.fired_frame = r, self.frames - 1
                break

    def advance(self, top_logp, top_idx, n):
        """top_logp / top_idx (T, k) arrays; the first n rows are real."""
        for t in range(max(0, min(int(n), len(top_logp)))):
            self.frame(top_logp[t][0], top_idx[t][0])

    def info(self):
        """A row of m3_ctc_endpoint_read."""
        return [self.frames, self.trailing_blank, self.decoded, self.first_speech, self.last_speech, self.fired_rule,
                self.fired_frame, 0]


def run(blank, log_thr, rules, calls, B):
    """calls: [(top_logp (B, T, k), top_idx (B, T, k), n_frames (B,))] in order -> info rows [B][8] after the last call."""
    refs = [EndpointRef(blank, log_thr, rules) for _ in range(B)]
    for lp, ix, nf in calls:
        for b in range(B):
            refs[b].advance(lp[b], ix[b], nf[b])
    return [r.info() for r in refs]
