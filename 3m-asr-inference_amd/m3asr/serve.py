"""Sessions that come and go on one batched streaming state: StreamPool, what a live service calls.

A pool owns the B slots of a slot-mode StreamingCtcDecoder (engine.streaming(B, max_frames, independent=True)).  Audio
arrives per session in pieces of any size; every `step()` is ONE engine call in which each session that has a window ready is
live and every other slot idle.

    pool = StreamPool(StreamingCtcDecoder(engine.streaming(B, max_frames, independent=True), beam=10))
    sid = pool.open()                       # takes a free slot, restarts it (open(context=graph_id): with hotwords;
                                            # open(lm=False): without the decoder's LM)
    pool.push(sid, frames)                  # (n, idim) feature frames, any n
    pool.end(sid)                           # no more audio for this session
    live = pool.step()                      # sids that moved one chunk
    best, greedy = pool.partial(sid)
    nbest = pool.close(sid)                 # frees the slot

Audio mode, `StreamPool(decoder, audio=True)`: sessions push SAMPLES (`pool.push_audio(sid, pcm)`, 16 kHz mono, int16 or
float32 in the int16 range).  step() gathers the live slots' sample windows into one pinned int16 buffer, uploads it once and
runs the log-Mel front end (m3asr.frontend.Fbank, one launch on the engine stream) straight into the encoder's window
buffer; the chunk itself is the same graph replay as in feature mode.

Delta features: when the engine's config has delta_order > 0 the front end is an m3asr.frontend.DeltaFbank and every
session's buffer keeps R = delta_order * delta_window frames of context: a window also carries up to R static frames in front
of and behind the frames it produces, and a frame is produced once its R frames of lookahead have arrived (or the stream has
ended).  That is R * 10 ms of added latency, one more launch per step and no host round trip; the frames are those of the
whole utterance featurised at once.

Audio at another rate or with several channels, `StreamPool(decoder, audio=True, sample_rate=44100, channels=2)`: the
sessions push interleaved samples in that format and step() resamples on the device (m3asr.frontend.Resampler, Kaldi's
LinearResample, one more launch) before the front end; a session's 16 kHz samples do not depend on how it was cut.

Segmenting, `StreamPool(decoder, segment=True)` over a decoder with an endpoint config
(StreamingCtcDecoder(..., endpoint=EndpointConfig())): after every step() the pool asks the device-side endpoint detector
which live sessions' utterances are over, files each one's n-best as a `Segment` (`pool.segments(sid)`) and restarts the
slot, so a session may stay open for any length of time inside a state sized for `max_frames`.

Two passes, `StreamPool(decoder, segment=True, rescore=True)` over a decoder with a rescorer
(StreamingCtcDecoder(..., endpoint=..., rescorer=AttentionRescorer(...))): when utterances end, ONE attention-decoder pass
rescores the n-best of all of them over the encoder memory the decoder kept per slot, and each is filed as a
`RescoredSegment`; `pool.close(sid, rescored=True)` does the same for the open segment.

Token times, `StreamPool(decoder, segment=True, timestamps=True)` over a decoder with an aligner
(StreamingCtcDecoder(..., endpoint=..., aligner=CtcAligner(...))): before a finished utterance's slot is restarted its final
best hypothesis is aligned to the logits the decoder kept for it, and the segment is filed as a `TimedSegment` whose `times`
are in session time; `pool.close(sid, timed=True)` does the same for the open segment.

The window rule is the one StreamingEncoder.decode applies to whole utterances (window n of a stream starts at its input
frame 4 c n, holds 4 c + 3 frames, overlaps the next by 3; fewer than 7 real frames count as none).  It lives in
`next_window_valid` / `WindowBuffer`, host-only code.
"""
import collections

import torch

from . import _lib

# One finished utterance of a segmenting pool's session.  rule: the endpoint rule that ended it (1-based); start_ms / end_ms:
# where its first and behind its last non-blank frame lie in the SESSION (the whole segment when no frame's argmax was a
# token); nbest: [(prefix, score)] best first, as close() returns; end_frame: the session's output frame at which the rule fired.
Segment = collections.namedtuple("Segment", "rule start_ms end_ms nbest end_frame")
# The same of a pool with rescore=True: the five fields of Segment, then best: the token tuple the attention decoder chose;
# scores: [(tokens, prior, att, final)] in n-best order (AttentionRescorer.rescore's pair).  Its memory is exactly the frames
# the n-best was searched over: the frames of the firing chunk behind the endpoint included.
RescoredSegment = collections.namedtuple("RescoredSegment", "rule start_ms end_ms nbest end_frame best scores")

# The same of a pool with timestamps=True: the seven fields of RescoredSegment (best / scores are None in a pool that does not
# rescore), then times: [(token, start_ms, end_ms, conf)] of the segment's final best hypothesis -- `best` with rescore=True,
# else the first n-best entry -- in SESSION time, (the segment's offset in frames + frame) * frame_ms; conf: the token's largest
# posterior inside its span; None when CTC cannot align the hypothesis (m3asr.align).
TimedSegment = collections.namedtuple("TimedSegment", "rule start_ms end_ms nbest end_frame best scores times")

# The same of a pool with words=True: the five fields of Segment, then what the graph search (m3asr.wfst) found on
# the segment's frames, read with the graph's final weights: words: word ids; word_ms: where each word's record was made, in
# SESSION time, (the segment's offset in frames + frame) * frame_ms; cost: the best token's cost; reached_final: whether that
# token stood on a final state.
WordSegment = collections.namedtuple("WordSegment", "rule start_ms end_ms nbest end_frame words word_ms cost reached_final")


def next_window_valid(buffered, chunks_done, chunk, ended):
    """Real frames in the next window of a stream, or 0 when that window cannot run yet (or never will).

    buffered: feature frames the stream has received since it began; chunks_done: windows already taken; chunk: c, output
    frames per chunk; ended: no more frames will come.  A window runs when it is full (4 c + 3 frames), or when the stream
    has ended and at least 7 frames remain from the window's start (the last, short window)."""
    window = 4 * chunk + 3
    left = buffered - 4 * chunk * chunks_done
    if left >= window:
        return window
    if ended and left >= 7:
        return left
    return 0


class WindowBuffer:
    """Feature frames of one stream, pushed in arbitrary pieces, handed back as the windows of chunked decoding."""

    def __init__(self, chunk, input_dim):
        self.c, self.idim = int(chunk), int(input_dim)
        self.window = 4 * self.c + 3
        self.buf = torch.zeros(0, self.idim)      # frames from input frame self.base on
        self.base = 0
        self.total = 0
        self.chunks = 0
        self.ended = False

    def push(self, frames):
        if self.ended:
            raise ValueError("push after end")
        frames = torch.as_tensor(frames, dtype=torch.float32).reshape(-1, self.idim).cpu()
        self.buf = torch.cat([self.buf, frames])
        self.total += int(frames.shape[0])

    def end(self):
        self.ended = True

    def rebase(self):
        """Start over at the next window: from here on the buffer behaves like a fresh one that was pushed every frame from
        input frame 4 c chunks on (the frames that window would read).  `ended` stays."""
        start = 4 * self.c * self.chunks
        self.buf = self.buf[min(max(start - self.base, 0), self.buf.shape[0]):]
        self.total = max(self.total - start, 0)
        self.base = 0
        self.chunks = 0

    def ready(self):
        """Real frames of the next window if it can run now, else 0."""
        return next_window_valid(self.total, self.chunks, self.c, self.ended)

    def drained(self):
        """The stream has ended and no further window will run."""
        return self.ended and self.ready() == 0

    def take(self, out=None):
        """The next window as (window (4c+3, idim) zero padded behind its real frames, valid); advances by one chunk."""
        valid = self.ready()
        if valid == 0:
            raise ValueError("no window ready")
        start = 4 * self.c * self.chunks - self.base
        win = torch.zeros(self.window, self.idim) if out is None else out
        win.zero_()
        win[:valid] = self.buf[start:start + valid]
        self.chunks += 1
        drop = 4 * self.c * self.chunks - self.base          # frames left of the next window are never read again
        if drop > 0:
            self.buf = self.buf[min(drop, self.buf.shape[0]):]
            self.base += drop
        return win, valid


class StreamPool:
    """B slots of a slot-mode streaming decoder shared by sessions that open and close at any time.

    decoder: a StreamingCtcDecoder over a slot-mode StreamingEncoder, or any object with `step(window (B, 4c+3, idim), valid
    (B,))`, `reset(slots=[...])`, `partial(slots=[...])`, `finish(slots=[...])`; B, chunk and input_dim are read from
    `decoder.st` unless given.  audio=True: the sessions are fed samples (push_audio) and step() featurises them on the device;
    fbank: the front end, `fbank(pcm (B, n) int16, n_samples (B,), out=, out_len=, stream=)` (default: an
    m3asr.frontend.Fbank for input_dim on the engine's device; a DeltaFbank when the engine's config has delta_order > 0, or
    any front end with a `context` attribute: it is then also passed lead= and n_out=).  sample_rate / channels / channel (audio=True): what the
    sessions push, one format per pool; unless they are 16000 / 1 / -1 every step() first runs ONE launch of `resampler`
    (default: an m3asr.frontend.Resampler for them on the engine's device; channel = -1: the mean of all channels, k: channel
    k alone) that turns the live slots' input spans into their 16 kHz float32 windows on the device, which the front end reads.

    segment=True: continuous decoding.  The decoder needs an endpoint config (`decoder.endpoint`, an
    m3asr.decode.EndpointConfig, and `decoder.endpoints(slots=[...])`).  After the engine call of a step() the pool reads the
    live slots' endpoint state -- the one host sync of a step.  For every slot whose rule fired it takes finish(slots=[b]),
    appends a Segment to the session unless the best hypothesis is empty, moves the session's offset on by the chunks the
    slot ran, restarts the slot (it keeps its hotword graph and LM setting) and rebases the session's buffer.  The session
    keeps its sid and goes on.  BOUNDARY: a rule fires at a frame, a slot moves by chunks: the frames of the firing chunk
    behind the endpoint stay with the finished segment (its n-best covers them), and the next segment starts at the next
    window -- it sees the three frames of overlap again but no encoder history from before.  segments(sid) hands out the
    finished segments, close(sid) the n-best of the open one, offset_ms(sid) where the open one starts.  With a rule that
    bounds an utterance's length (the default third rule) no slot reaches max_frames; that needs min_length + c <= max_frames
    (max_frames is read from `decoder.st` unless given).

    rescore=True: two-pass decoding.  The decoder needs a rescorer (`decoder.rescorer`, `decoder.rescore(slots=[...],
    detail=True)`).  With segment=True all slots whose rule fired in a step are rescored by ONE decoder.rescore call before
    they are restarted, and segments(sid) hands out RescoredSegments; close(sid, rescored=True) rescores the open segment.

    timestamps=True: token times.  The decoder needs an aligner (`decoder.aligner`, `decoder.align(slots=[...],
    tokens=[...])`) and the pool must segment (the times are session times, frame_ms is the endpoint config's).  All slots whose
    rule fired in a step are aligned by ONE decoder.align call before they are restarted, and segments(sid) hands out
    TimedSegments; close(sid, timed=True) aligns the open segment.

    words=True: graph decoding.  The decoder needs a graph (`decoder.graph`, `decoder.words(slots=[...], final=, detail=)`:
    StreamingCtcDecoder(..., graph=DecodingGraph(...))).  words(sid) reads the open segment's words and their session times.
    With segment=True all slots whose rule fired in a step are read by ONE decoder.words(final=True, detail=True) call before
    any is restarted, segments(sid) hands out WordSegments, and a segment is filed when its best prefix OR its word list is not
    empty.  Not together with rescore=True or timestamps=True: the second pass needs token hypotheses out of the graph."""

    def __init__(self, decoder, B=None, chunk=None, input_dim=None, audio=False, fbank=None, segment=False, max_frames=None,
                 rescore=False, timestamps=False, sample_rate=16000, channels=1, channel=-1, resampler=None, words=False):
        self.dec = decoder
        self.rescore = bool(rescore)
        self.timestamps = bool(timestamps)
        self.with_words = bool(words)
        if self.with_words and (getattr(decoder, "graph", None) is None or not hasattr(decoder, "words")):
            raise _lib.M3Error("StreamPool(words=True) needs a decoder with a graph: "
                               "StreamingCtcDecoder(..., graph=DecodingGraph(...))")
        if self.with_words and (self.rescore or self.timestamps):
            raise _lib.M3Error("StreamPool(words=True) does not go with %s=True: the second pass and the aligner need token "
                               "hypotheses, which the graph search does not give" % ("rescore" if self.rescore else "timestamps"))
        if self.timestamps and (getattr(decoder, "aligner", None) is None or not hasattr(decoder, "align")):
            raise _lib.M3Error("StreamPool(timestamps=True) needs a decoder with an aligner: "
                               "StreamingCtcDecoder(..., aligner=CtcAligner(...))")
        if self.timestamps and not segment:
            raise _lib.M3Error("StreamPool(timestamps=True) needs segment=True: token times are session times")
        if self.rescore and (getattr(decoder, "rescorer", None) is None or not hasattr(decoder, "rescore")):
            raise _lib.M3Error("StreamPool(rescore=True) needs a decoder with a rescorer: "
                               "StreamingCtcDecoder(..., rescorer=AttentionRescorer(...))")
        st = getattr(decoder, "st", None)
        if st is not None and not getattr(st, "independent", False):
            raise _lib.M3Error("StreamPool needs a slot-mode encoder: engine.streaming(B, max_frames, independent=True)")
        self.B = int(B if B is not None else st.desc.B)
        self.c = int(chunk if chunk is not None else st.c)
        self.idim = int(input_dim if input_dim is not None else st.feat.shape[2])
        self.window = 4 * self.c + 3
        self.slot_sid = [None] * self.B          # who holds slot b
        self.streams = {}                        # sid -> (slot, WindowBuffer)
        self.next_sid = 0
        self.win = torch.zeros(self.B, self.window, self.idim)
        self.steps = 0
        self.segment = bool(segment)
        if self.segment:
            ep = getattr(decoder, "endpoint", None)
            if ep is None or not hasattr(decoder, "endpoints"):
                raise _lib.M3Error("StreamPool(segment=True) needs a decoder with an endpoint config: "
                                   "StreamingCtcDecoder(..., endpoint=EndpointConfig())")
            self.frame_ms = int(ep.frame_ms)
            if max_frames is None and st is not None:
                max_frames = st.desc.max_frames
            bound = ep.length_bound()
            if max_frames is not None and bound is not None and bound + self.c > int(max_frames):
                raise _lib.M3Error("StreamPool(segment=True): the length rule fires at %d frames, a slot may then stand at up "
                                   "to %d + c = %d > max_frames = %d" % (bound, bound, bound + self.c, int(max_frames)))
            self.offset = {}                     # sid -> output frames of the session before its open segment
            self.finished = {}                   # sid -> [Segment] not handed out yet
        elif self.with_words:                    # word times of a pool that does not segment: the session is one segment
            ep = getattr(decoder, "endpoint", None)
            self.frame_ms = int(ep.frame_ms) if ep is not None else 40
        self.audio = bool(audio)
        self.sample_rate, self.channels, self.channel = int(sample_rate), int(channels), int(channel)
        self.resampled = self.audio and (self.sample_rate, self.channels, self.channel) != (16000, 1, -1)
        if not self.audio and (self.sample_rate, self.channels, self.channel) != (16000, 1, -1):
            raise ValueError("StreamPool: sample_rate / channels / channel belong to a pool fed samples (audio=True)")
        if self.audio:
            self._init_audio(st, fbank)
        if self.resampled:
            self._init_resampler(st, resampler)

    def _init_resampler(self, st, resampler):
        """The buffers of a pool whose sessions push samples at another rate or with several channels: per slot the input
        span of a window (pinned, then device) and ONE index block (in0, out0 int64; n_in, n_out int32) that goes up in one
        copy; the resampler writes the 16 kHz windows as float32 into res_dev, which the front end reads."""
        from .frontend import AudioWindowBuffer, Resampler
        self._new_audio_buffer = lambda: AudioWindowBuffer(self.c, sample_rate=self.sample_rate, channels=self.channels,
                                                           context=self.context)
        eng = getattr(st, "eng", None)
        dev = eng.device if eng is not None else torch.device("cpu")
        pin = dev.type == "cuda"
        self.resampler = resampler if resampler is not None else Resampler(self.sample_rate, dev, channels=self.channels,
                                                                           channel=self.channel)
        B, width = self.B, -(-self._new_audio_buffer().span * self.channels // 8) * 8
        self.span_win = torch.zeros(B, width, dtype=torch.int16, pin_memory=pin)
        self.span_dev = torch.zeros(B, width, dtype=torch.int16, device=dev)
        self.idx = torch.zeros(3 * B, dtype=torch.int64, pin_memory=pin)         # in0 | out0 | n_in, n_out (int32 pairs)
        self.idx_dev = torch.zeros(3 * B, dtype=torch.int64, device=dev)
        self.res_dev = torch.zeros(B, self.window_samples, dtype=torch.float32, device=dev)

    def _index_views(self, idx):
        B = self.B
        n = idx[2 * B:].view(torch.int32)
        return idx[:B], n[:B], idx[B:2 * B], n[B:]

    def _init_audio(self, st, fbank):
        from .frontend import AudioWindowBuffer, Fbank, make_frontend
        eng = getattr(st, "eng", None)
        if fbank is None:
            fbank = make_frontend(eng.cfg, eng.device) if getattr(eng, "cfg", None) is not None else Fbank(self.idim, eng.device)
        self.fbank = fbank
        self.context = int(getattr(fbank, "context", 0))        # frames of context a delta front end reads on either side
        self._new_audio_buffer = lambda: AudioWindowBuffer(self.c, context=self.context)
        self.stream = eng.stream if eng is not None else None
        dev = eng.device if eng is not None else torch.device("cpu")
        pin = dev.type == "cuda"
        self.window_samples = self._new_audio_buffer().window
        self.pcm_win = torch.zeros(self.B, self.window_samples, dtype=torch.int16, pin_memory=pin)
        # per slot: real samples | frames of context in front | frames to produce -- one upload
        self.counts = torch.zeros(3, self.B, dtype=torch.int32, pin_memory=pin)
        self.counts_dev = torch.zeros(3, self.B, dtype=torch.int32, device=dev)
        self.n_real, self.n_real_dev = self.counts[0], self.counts_dev[0]
        self.pcm_dev = torch.zeros(self.B, self.window_samples, dtype=torch.int16, device=dev)
        self.feat_len_dev = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.feat = st.feat if st is not None else self.win      # where the frames land: the encoder's own window buffer
        self.uploaded = torch.cuda.Event() if pin else None     # the pinned buffers may be refilled once this has passed

    def _get(self, sid):
        if sid not in self.streams:
            raise KeyError("StreamPool: no open stream %r" % (sid,))
        return self.streams[sid]

    def free_slots(self):
        return sum(1 for s in self.slot_sid if s is None)

    def slot_of(self, sid):
        return self._get(sid)[0]

    def open(self, context=None, lm=None):
        """Take a free slot and restart it; -> stream id.  Raises M3Error when all B slots are taken.
        context: graph id in the decoder's ContextSet for this session's beam search (None = unbiased).
        lm: whether this session's beam search runs with the decoder's LM (None = yes if the decoder has one).  A decoder built
        with an NgramLmSet takes an int as well: lm=j is member j - 1 of the set (True / 1 / None: member 0), 0 / False none;
        the segments a session is cut into all keep its member."""
        biased = getattr(self.dec, "context", None) is not None
        fused = getattr(self.dec, "lm", None) is not None
        if context is not None and not biased:
            raise _lib.M3Error("StreamPool.open: the decoder was built without a context")
        if lm and not fused:
            raise _lib.M3Error("StreamPool.open: the decoder was built without an LM")
        for b, holder in enumerate(self.slot_sid):
            if holder is None:
                kw = {}
                if biased:
                    kw["graph_ids"] = [-1 if context is None else int(context)]
                if fused:
                    kw["lm_on"] = [1 if lm is None else int(lm)]   # True = 1: the LM, or member 0 of a set; an id above the set is refused
                self.dec.reset(slots=[b], **kw)
                sid = self.next_sid
                self.next_sid += 1
                self.slot_sid[b] = sid
                self.streams[sid] = (b, self._new_audio_buffer() if self.audio else WindowBuffer(self.c, self.idim))
                if self.segment:
                    self.offset[sid], self.finished[sid] = 0, []
                return sid
        raise _lib.M3Error("StreamPool.open: all %d slots are taken" % self.B)

    def push(self, sid, frames):
        if self.audio:
            raise ValueError("StreamPool.push: this pool is fed samples (audio=True), use push_audio")
        self._get(sid)[1].push(frames)

    def push_audio(self, sid, pcm):
        """Samples of the stream, any number: int16 or float32 in the int16 value range, at the POOL's sample_rate (16 kHz unless
        the pool was built with another) and with the pool's channels, (n, channels) or interleaved (n * channels,); mono
        pools take (n,).  A pool at another rate or with several channels resamples on the device (Kaldi's LinearResample,
        DESIGN.md 31), so the session's 16 kHz samples are those of the whole session resampled at once, however it is cut."""
        if not self.audio:
            raise ValueError("StreamPool.push_audio: this pool is fed feature frames, build it with audio=True")
        self._get(sid)[1].push(pcm)

    def end(self, sid):
        self._get(sid)[1].end()

    def pending(self, sid):
        """True while the stream has a window that step() would run."""
        return self._get(sid)[1].ready() > 0

    def step(self):
        """ONE engine call: every stream with a full window buffered (or ended with >= 7 frames left) moves one chunk, every
        other slot is idle.  -> the sids that were live (no call at all when there is none)."""
        if self.audio:
            return self._step_audio()
        valid = torch.zeros(self.B, dtype=torch.int32)
        live = []
        for sid, (b, wb) in self.streams.items():
            if wb.ready() > 0:
                _, v = wb.take(out=self.win[b])
                valid[b] = v
                live.append(sid)
        if live:
            self.dec.step(self.win, valid)
            self.steps += 1
            if self.segment:
                self._cut(live)
        return live

    def _cut(self, live):
        """segment=True, after the engine call: end the utterance of every live session whose endpoint rule fired."""
        slots = [self.streams[sid][0] for sid in live]
        fired = [(sid, b, info) for sid, b, info in zip(live, slots, self.dec.endpoints(slots=slots)) if info.rule]
        if not fired:
            return
        # two passes: one decoder pass over everything that ended in this step, before any of the slots is restarted
        second = self.dec.rescore(slots=[b for _, b, _ in fired], detail=True) if self.rescore else None
        times = None
        if self.timestamps:               # one alignment pass over everything that ended in this step, likewise
            nbests = [self.dec.finish(slots=[b])[0] for _, b, _ in fired]
            times = self._times(fired, nbests, second)
        # graph decoding: one read of every finished slot's words, likewise
        found = self.dec.words(slots=[b for _, b, _ in fired], final=True, detail=True) if self.with_words else None
        for j, (sid, b, info) in enumerate(fired):
            nbest = nbests[j] if times is not None else self.dec.finish(slots=[b])[0]
            buf, off = self.streams[sid][1], self.offset[sid]
            if (nbest and len(nbest[0][0]) > 0) or (found is not None and found[j]["words"]):
                first = info.first_speech if info.first_speech >= 0 else 0
                last = info.last_speech if info.last_speech >= 0 else info.frame
                seg = Segment(info.rule, (off + first) * self.frame_ms, (off + last + 1) * self.frame_ms, nbest, off + info.frame)
                if second is not None:
                    seg = RescoredSegment(*seg, tuple(second[j][0]), second[j][1])
                if times is not None:
                    seg = TimedSegment(*(tuple(seg) + (None, None))[:7], times[j])
                if found is not None:
                    w = found[j]
                    seg = WordSegment(*seg, list(w["words"]), [(off + f) * self.frame_ms for f in w["frames"]], w["cost"],
                                      w["reached_final"])
                self.finished[sid].append(seg)
            self.offset[sid] = off + buf.chunks * self.c
            self.dec.reset(slots=[b])
            buf.rebase()

    def _times(self, fired, nbests, second):
        """timestamps=True: ONE decoder.align call over the slots of `fired` [(sid, slot, ...)], each on its final best
        hypothesis (the second pass's choice when there was one, else the first n-best entry) -> per entry
        [(token, start_ms, end_ms, conf)] in session time, or None where there is no alignment."""
        from .align import token_times
        tokens = [list(second[j][0]) if second is not None else (list(nbest[0][0]) if nbest else [])
                  for j, nbest in enumerate(nbests)]
        got = self.dec.align(slots=[f[1] for f in fired], tokens=tokens)
        return [token_times(a, self.frame_ms, self.offset[f[0]]) for f, a in zip(fired, got)]

    def segments(self, sid):
        """The session's finished segments since the last call, oldest first (segment=True); the list is cleared."""
        if not self.segment:
            raise ValueError("StreamPool.segments: this pool does not segment, build it with segment=True")
        self._get(sid)
        out, self.finished[sid] = self.finished[sid], []
        return out

    def offset_ms(self, sid):
        """Where in the session its open segment starts, in ms (segment=True)."""
        if not self.segment:
            raise ValueError("StreamPool.offset_ms: this pool does not segment, build it with segment=True")
        self._get(sid)
        return self.offset[sid] * self.frame_ms

    def _step_audio(self):
        """step() of a pool fed samples: one small int16 upload, one front-end launch into the encoder's window buffer, then
        the chunk.  An idle slot has 0 samples: its rows of the window buffer are zeroed and its `valid` is 0."""
        if self.resampled:
            return self._step_resampled()
        if self.uploaded is not None:
            self.uploaded.synchronize()
        valid = torch.zeros(self.B, dtype=torch.int32)
        self.counts.zero_()
        live = []
        for sid, (b, ab) in self.streams.items():
            v = ab.ready()
            if v > 0:
                _, n = ab.take(out=self.pcm_win[b])
                self.counts[0, b], self.counts[1, b], self.counts[2, b] = n, ab.lead, v
                valid[b] = v
                live.append(sid)
        if not live:
            return live
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                self.pcm_dev.copy_(self.pcm_win, non_blocking=True)
                self.counts_dev.copy_(self.counts, non_blocking=True)
                self.uploaded.record(self.stream)
        else:
            self.pcm_dev.copy_(self.pcm_win)
            self.counts_dev.copy_(self.counts)
        self._featurise(self.pcm_dev, self.n_real_dev)
        self.dec.step(self.feat, valid)
        self.steps += 1
        if self.segment:
            self._cut(live)
        return live

    def _featurise(self, pcm_dev, n_dev):
        """The front-end launch(es) of a step into the encoder's window buffer; with delta features the windows carry
        counts_dev[1] frames of context in front and counts_dev[2] frames are produced."""
        if self.context > 0:
            self.fbank(pcm_dev, n_dev, out=self.feat, out_len=self.feat_len_dev, stream=self.stream, lead=self.counts_dev[1],
                       n_out=self.counts_dev[2])
        else:
            self.fbank(pcm_dev, n_dev, out=self.feat, out_len=self.feat_len_dev, stream=self.stream)

    def _step_resampled(self):
        """step() of a pool fed samples at another rate: the live slots' input spans and the index block go up, ONE resampler
        launch writes every slot's 16 kHz window (an idle slot has n_out = 0: zeros), then the front end and the chunk run
        as in _step_audio.  One launch more per step, no host round trip."""
        from .frontend import num_frames
        if self.uploaded is not None:
            self.uploaded.synchronize()
        valid = torch.zeros(self.B, dtype=torch.int32)
        self.idx.zero_()
        self.counts.zero_()
        in0, n_in, out0, n_out = self._index_views(self.idx)
        live = []
        for sid, (b, ab) in self.streams.items():
            v = ab.ready()
            if v > 0:
                _, in0[b], n_in[b], out0[b], n_out[b] = ab.take(out=self.span_win[b, :ab.span * self.channels])
                assert num_frames(int(n_out[b])) >= v and (self.context > 0 or num_frames(int(n_out[b])) == v)
                self.counts[1, b], self.counts[2, b] = ab.lead, v
                valid[b] = v
                live.append(sid)
        if not live:
            return live
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                self.span_dev.copy_(self.span_win, non_blocking=True)
                self.idx_dev.copy_(self.idx, non_blocking=True)
                if self.context > 0:
                    self.counts_dev.copy_(self.counts, non_blocking=True)
                self.uploaded.record(self.stream)
        else:
            self.span_dev.copy_(self.span_win)
            self.idx_dev.copy_(self.idx)
            self.counts_dev.copy_(self.counts)
        d_in0, d_n_in, d_out0, d_n_out = self._index_views(self.idx_dev)
        self.resampler.launch(self.span_dev, d_in0, d_n_in, d_out0, d_n_out, self.res_dev, stream=self.stream)
        self._featurise(self.res_dev, d_n_out)
        self.dec.step(self.feat, valid)
        self.steps += 1
        if self.segment:
            self._cut(live)
        return live

    def partial(self, sid):
        """(best beam hypothesis (prefix, score), greedy tokens) of the stream so far."""
        b = self.slot_of(sid)
        best, greedy = self.dec.partial(slots=[b])
        return best[0], greedy[0]

    def words(self, sid, final=False):
        """(word ids, word_ms) of what the graph search has found in the stream so far (segment=True: in its open segment);
        word_ms in session time, (the open segment's offset in frames + the word's frame) * frame_ms (the endpoint config's,
        40 without one).  final: the graph's final weights count, as at an utterance's end (words=True)."""
        b = self.slot_of(sid)
        if not self.with_words:
            raise _lib.M3Error("StreamPool.words: this pool does not decode through a graph, build it with words=True")
        w = self.dec.words(slots=[b], final=final, detail=True)[0]
        off = self.offset[sid] if self.segment else 0
        return list(w["words"]), [(off + f) * self.frame_ms for f in w["frames"]]

    def close(self, sid, rescored=False, timed=False):
        """n-best [(prefix, score)] of what the stream has decoded (segment=True: of its open segment; read segments(sid)
        first, the finished ones go with the session); the slot is free again.
        rescored=True (rescore=True): instead the second pass's pair for it, (best tokens, [(tokens, prior, att, final)]);
        ((), []) when nothing was decoded.
        timed=True (timestamps=True): (that result, times) -- times as in TimedSegment, of the second pass's choice with
        rescored=True and of the first n-best entry otherwise."""
        b = self.slot_of(sid)
        if timed and not self.timestamps:
            raise _lib.M3Error("StreamPool.close(timed=True): this pool keeps no token times, build it with timestamps=True")
        if rescored:
            if not self.rescore:
                raise _lib.M3Error("StreamPool.close(rescored=True): this pool does not rescore, build it with rescore=True")
            best, scores = self.dec.rescore(slots=[b], detail=True)[0]
            nbest = (tuple(best), scores)
        else:
            nbest = self.dec.finish(slots=[b])[0]
        if timed:
            fired = [(sid, b)]
            nbest = (nbest, self._times(fired, [[] if rescored else nbest], [nbest] if rescored else None)[0])
        del self.streams[sid]
        if self.segment:
            del self.offset[sid], self.finished[sid]
        self.slot_sid[b] = None
        return nbest
