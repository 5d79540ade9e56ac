"""Long recordings through a full-context engine: energy VAD on the signal, segments batched into the engine.

A full-context encoder refuses an utterance whose subsampled length reaches its positional table (cfg.max_len, about 200 s),
and its attention grows with T'^2.  A streaming model is cut at CTC blank runs (StreamPool(segment=True)), which needs the
encoder to have run; a full-context model has to be cut BEFORE the encoder runs, and the only place for that is the signal.

    lf = LongFormTranscriber(engine)                                   # VadConfig() defaults
    for seg in lf.transcribe(pcm, sample_rate=44100, channels=2, mode="greedy", timestamps=True):
        print(seg.start_ms, seg.end_ms, seg.tokens, seg.times)

The features are computed once over the whole recording and then cut (m3_segment_gather): a segment's delta columns at its
edges come from the real neighbouring frames.  Every launch runs on the engine's stream; per batch the host uploads one job
list and replays the shape's graph.  `plan_batches` is pure Python and needs no GPU.
"""
import collections

import torch

from .config import subsampled_len
from .frontend import (FRAME_LENGTH, FRAME_MS, FRAME_SHIFT, EnergyVad, Fbank, VadConfig, add_deltas, make_frontend, num_frames,
                       segment_gather)

# One segment of a recording: its span in ms of the 16 kHz signal (frame k starts at 10 k ms), its tokens, and with
# timestamps=True its [(token, start_ms, end_ms, conf)] on the recording's clock (None when CTC cannot align the tokens).
LongSegment = collections.namedtuple("LongSegment", "start_ms end_ms tokens times")
LongSegment.__new__.__defaults__ = (None,)

MIN_FRAMES = 7                        # the encoder's shortest input: fewer frames give no output frame
OUT_FRAME_MS = 4 * FRAME_MS           # Conv2dSubsampling4


def _round_up(n, m):
    return -(-int(n) // int(m)) * int(m)


class LongFormTranscriber:
    """engine: a full-context m3asr.engine.Engine.  vad: VadConfig.  A batch holds at most max_batch segments and at most
    max_batch_frames padded frames (default: four segments of the longest kind); its frame count is rounded up to a multiple
    of `bucket`, so a recording binds a bounded number of (B, T) shapes in the engine's LRU."""

    def __init__(self, engine, vad=None, max_batch=16, max_batch_frames=None, bucket=100, blank_idx=0, rescorer=None):
        self.engine, self.cfg = engine, engine.cfg
        self.vad_cfg = VadConfig() if vad is None else vad
        self.max_batch, self.bucket = int(max_batch), int(bucket)
        if self.max_batch < 1 or self.bucket < 1:
            raise ValueError("LongFormTranscriber: max_batch=%d, bucket=%d: both must be at least 1" % (self.max_batch, self.bucket))
        longest = _round_up(self.vad_cfg.max_segment, self.bucket)
        if subsampled_len(longest) >= self.cfg.max_len:
            raise ValueError("LongFormTranscriber: max_segment=%d frames (%d in a batch) subsample to %d, the positional table has "
                             "%d rows" % (self.vad_cfg.max_segment, longest, subsampled_len(longest), self.cfg.max_len))
        self.max_batch_frames = 4 * longest if max_batch_frames is None else int(max_batch_frames)
        if self.max_batch_frames < longest:
            raise ValueError("LongFormTranscriber: max_batch_frames=%d cannot hold one segment of %d frames" % (self.max_batch_frames, longest))
        self.device = engine.device
        self.frontend = make_frontend(self.cfg, self.device)
        self.vad = EnergyVad(self.vad_cfg, self.device)
        self.blank_idx, self.rescorer = int(blank_idx), rescorer
        self._decoder = self._aligner = None
        self.piece_frames = 1 << 25          # log-Mel frames per m3_fbank launch (its grid takes fewer than 2^26)

    # ---- host side -----------------------------------------------------------------------
    def plan_batches(self, segments):
        """segments: [(start, end)] in frames -> [(indices into `segments`, T_max)]: sorted by length, longest first (equal
        lengths in list order), batches filled greedily while B <= max_batch and B * T_max <= max_batch_frames, T_max = the
        batch's longest segment rounded up to a multiple of `bucket`.  Every segment appears exactly once."""
        order = sorted(range(len(segments)), key=lambda i: (-(segments[i][1] - segments[i][0]), i))
        out, i = [], 0
        while i < len(order):
            n = segments[order[i]][1] - segments[order[i]][0]
            if n < 1:
                raise ValueError("plan_batches: segment %d is empty: %s" % (order[i], (segments[order[i]],)))
            T_max = _round_up(n, self.bucket)
            if T_max > self.max_batch_frames:
                raise ValueError("plan_batches: segment %d of %d frames exceeds max_batch_frames=%d" % (order[i], n, self.max_batch_frames))
            B = min(self.max_batch, self.max_batch_frames // T_max, len(order) - i)
            out.append((order[i:i + B], T_max))
            i += B
        return out

    # ---- device side ---------------------------------------------------------------------
    def _signal(self, pcm, sample_rate, channels, channel):
        """One recording -- (N,), (1, N); with channels > 1 (N, channels), (1, N, channels) or interleaved -- as the launches
        read it: (samples (1, ld) on the device, int16 or float32; n (1,) int32 on the device; N on the host).  Staged, and
        resampled unless it is 16 kHz mono, ONCE on the engine's stream: the features and the VAD read the same tensor."""
        pcm = torch.as_tensor(pcm)
        channels = int(channels)
        pcm = pcm.reshape(1, -1) if channels == 1 else pcm.reshape(1, -1, channels)
        if (int(sample_rate), channels, int(channel)) != (16000, 1, -1):
            return self.engine._resampled(pcm, None, int(sample_rate), channels, int(channel))
        with torch.cuda.device(self.device), torch.cuda.stream(self.engine.stream):
            dev, N = Fbank._device_pcm(self, pcm)
            return dev, torch.full((1,), N, dtype=torch.int32, device=self.device), N

    def features(self, pcm, sample_rate=16000, channels=1, channel=-1, _signal=None):
        """One recording -> its (T_all, input_dim) feature frames on the device: resampled first unless it is 16 kHz mono, then
        log-Mel (and deltas) over the WHOLE recording, so every frame's delta columns see their real neighbours.  One launch of
        m3_fbank takes fewer than 2^26 frames (its grid); a longer recording's log-Mel frames are computed `piece_frames` at a
        time into their rows -- a frame depends on its own 400 samples only -- and the deltas then run once over all rows in
        place: the same bits as one call."""
        sig, n, N = self._signal(pcm, sample_rate, channels, channel) if _signal is None else _signal
        T_all, fb, st = num_frames(N), self.frontend, self.engine.stream
        out = torch.empty(1, T_all, self.cfg.input_dim, dtype=torch.float32, device=self.device)
        if T_all <= self.piece_frames:
            fb(sig, n, out=out, stream=st)
            return out[0]
        static = getattr(fb, "fbank", fb)                          # DeltaFbank: its Fbank
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            for t0 in range(0, T_all, self.piece_frames):
                t1 = min(t0 + self.piece_frames, T_all)
                first, last = FRAME_SHIFT * t0, FRAME_SHIFT * (t1 - 1) + FRAME_LENGTH      # 160 samples are whole 16 bytes
                static(sig[:, first:], torch.full((1,), last - first, dtype=torch.int32, device=self.device), out=out[:, t0:t1], stream=st)
            if static is not fb:
                add_deltas(out, torch.full((1,), T_all, dtype=torch.int32, device=self.device), fb.order, fb.delta_window, out=out,
                           bins=fb.bins, stream=st)
        return out[0]

    def segment(self, pcm, sample_rate=16000, channels=1, channel=-1):
        """-> ([(start, end)] in frames, features (T_all, input_dim) on the device)"""
        sig = self._signal(pcm, sample_rate, channels, channel)
        feat = self.features(None, _signal=sig)
        segs = self.vad(sig[0], sig[1], stream=self.engine.stream)[0] if feat.shape[0] else []
        return segs, feat

    def batches(self, pcm, sample_rate=16000, channels=1, channel=-1, _segmented=None):
        """Generator over the planned batches of one recording: (indices into the segment list, logits (B, T', V) of the
        engine's static output buffer for the shape -- valid until the next batch --, out_lens (B,) int32 on the device).
        Segments shorter than the encoder's 7 frames are in no batch."""
        segs, feat = self.segment(pcm, sample_rate, channels, channel) if _segmented is None else _segmented
        eng = self.engine
        keep = [i for i, (s, e) in enumerate(segs) if e - s >= MIN_FRAMES]
        for idx, T in self.plan_batches([segs[i] for i in keep]):
            idx = [keep[i] for i in idx]
            B = len(idx)
            f, l, out = eng._lru(eng._static, (B, T), lambda: (
                torch.empty(B, T, self.cfg.input_dim, dtype=torch.float32, device=self.device),
                torch.empty(1, B, dtype=torch.int32, device=self.device),
                torch.empty(eng.output_shape(B, T), dtype=torch.float32, device=self.device)))
            with torch.cuda.stream(eng.stream):
                jobs = torch.tensor([(0, segs[i][0], segs[i][1]) for i in idx], dtype=torch.int32).to(self.device)
            segment_gather(feat, jobs, f, l, cols=self.cfg.input_dim, stream=eng.stream)
            eng.forward(f, l, out, use_graph=True)
            eng.stream.synchronize()
            yield idx, out, eng.buffer("lens", torch.int32)[:B].clone()

    # ---- decoding ------------------------------------------------------------------------
    def _mode(self, mode, kw):
        from .decode import CtcDecoder
        if self._decoder is None:
            self._decoder = CtcDecoder(self.engine, self.blank_idx, rescorer=self.rescorer)
        dec = self._decoder
        if mode == "greedy":
            return lambda logits, lens, hidden: dec.greedy_from_logits(logits, lens)
        beam = int(kw.pop("beam_size", 10))
        first = lambda hyps: [list(h[0][0]) if h else [] for h in hyps]                       # noqa: E731
        if mode == "beam":
            return lambda logits, lens, hidden: first(dec.batch_prefix_beam_from_logits(logits, lens, beam, **kw))
        if mode == "rescore":
            return lambda logits, lens, hidden: dec.rescore_from_logits(logits, lens, beam, **kw)
        if mode == "attention":
            return lambda logits, lens, hidden: dec.attention_from_logits(logits, lens, beam, **kw)
        raise ValueError("LongFormTranscriber: mode %r, need 'greedy', 'beam', 'rescore' or 'attention'" % (mode,))

    def _times(self, logits, lens, tokens, starts_ms):
        """CTC alignment of the batch's non-empty hypotheses; token times shifted to the recording's clock"""
        from .align import CtcAligner
        B, Tp, V = logits.shape
        if self._aligner is None or self._aligner.V != V:
            self._aligner = CtcAligner(V, self.blank_idx, self.device, OUT_FRAME_MS)
        live = [b for b in range(B) if tokens[b]]
        got = self._aligner.align_rows(logits.reshape(B * Tp, V), [b * Tp for b in live], [lens[b] for b in live],
                                       [tokens[b] for b in live])
        out = [None if tokens[b] else [] for b in range(B)]
        for b, a in zip(live, got):
            if a.ok:
                out[b] = [(tok, starts_ms[b] + s, starts_ms[b] + e, c) for tok, s, e, c in zip(a.tokens, a.start_ms, a.end_ms, a.conf)]
        return out

    def transcribe(self, pcm, sample_rate=16000, channels=1, channel=-1, decode=None, mode="greedy", timestamps=False, **kw):
        """-> [LongSegment] in time order.  decode(logits (B, T', V), out_lens (B,), hidden or None) -> one token list per row;
        without it mode = "greedy" | "beam" | "rescore" | "attention" forwards to CtcDecoder's *_from_logits entry points with
        the keyword arguments given here (beam_size, lm, lm_weight, length_bonus, context, ctc_weight, ...); the last two need
        a rescorer (LongFormTranscriber(rescorer=AttentionRescorer(...))).  A decode function that wants the encoder's hidden
        states sets `decode.needs_hidden = True`.  timestamps: CtcAligner per batch; each token's times are shifted by its
        segment's start, the way TimedSegment carries session times."""
        fn = self._mode(mode, dict(kw)) if decode is None else decode
        segs, feat = self.segment(pcm, sample_rate, channels, channel)
        ms = FRAME_MS
        tokens, times = [[] for _ in segs], [[] if timestamps else None for _ in segs]
        for idx, logits, out_lens in self.batches(None, _segmented=(segs, feat)):
            hidden = self.engine.hidden() if getattr(fn, "needs_hidden", False) else None
            got = [list(t) for t in fn(logits, out_lens, hidden)]
            if len(got) != len(idx):
                raise ValueError("LongFormTranscriber: decode returned %d token lists for a batch of %d" % (len(got), len(idx)))
            when = self._times(logits, out_lens.cpu().tolist(), got, [segs[i][0] * ms for i in idx]) if timestamps else None
            for b, i in enumerate(idx):
                tokens[i] = got[b]
                if timestamps:
                    times[i] = when[b]
        return [LongSegment(s * ms, e * ms, tokens[i], times[i]) for i, (s, e) in enumerate(segs)]
