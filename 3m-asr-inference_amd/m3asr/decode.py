"""CTC searches behind the encoder engine -- host mirror of the reference's decoding entry points
(trainer_3m_fix/model/encoder.py:156-275: `ctc_greedy_search`, `ctc_prefix_beam_search`; same names, argument meaning
and return types), running on the device through libm3asr_hip.so:

  greedy        logits stay on the GPU; argmax + repeat/blank collapse are kernels (m3_ctc_greedy); only the token
                lists (B x T' int32 + counts) are copied back.
  prefix beam   per-frame log-softmax + top-`beam` on the GPU (m3_ctc_topk), T' x beam pairs copied back, the prefix
                recursion in the library's host routine (m3_ctc_prefix_beam_search).
  batched beam  B utterances in one device search (m3_ctc_topk + m3_ctc_beam_advance + m3_ctc_beam_nbest): CtcBeamSearch,
                CtcDecoder.batch_prefix_beam_search; resumable chunk by chunk, which StreamingCtcDecoder uses on top of the
                chunk-by-chunk engine (with the streaming greedy search, m3_ctc_greedy_stream_*).
  endpoints     when an utterance of a live stream is over (m3_ctc_endpoint_*): EndpointConfig, and
                StreamingCtcDecoder(endpoint=...).endpoints(); m3asr.serve.StreamPool(segment=True) cuts sessions there.
  rescoring     the reference's second pass (model/ctc_aed.py:160-252): CtcDecoder(engine, rescorer=...).attention_rescoring
                runs the batched beam search, then the attention decoder over its n-best (m3asr.rescore).
  attention     CtcDecoder(engine, rescorer=...).attention: the attention decoder's own beam search (m3asr.aed_search).
  two passes,   StreamingCtcDecoder(..., rescorer=...) keeps every stream's encoder memory on the device (m3_aed_memory_*) and
  streaming     rescore() runs the second pass over a stream's n-best when its utterance ends; StreamPool(rescore=True).

  graph         CtcDecoder.ctc_wfst_search: token passing over a compiled decoding graph (TLG) -- word LMs, a closed vocabulary,
                pronunciation variants -- returning words (m3_wfst_*, m3asr.wfst: DecodingGraph, CtcWfstSearch).

  token times   when each token of a hypothesis was spoken (m3_ctc_align_*, m3asr.align): CtcDecoder.align for the hypotheses of
                any mode above, StreamingCtcDecoder(..., aligner=CtcAligner(...)).align() on the logits the decoder kept per
                stream; StreamPool(timestamps=True).

Chunked decoding (decoding_chunk_size > 0) is accepted when the engine was built for exactly that chunk mask
(cfg.static_chunk_size == decoding_chunk_size, same num_decoding_left_chunks): its ordinary forward is then the reference's
chunk-masked forward (encoder.py:100-140).

There is no CPU fallback: without the HIP library every call raises.
"""
import collections
import math
from typing import List, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import lm as _lm
from .config import subsampled_len


def _same_device(a, b):
    """torch.device("cuda") names the current device and a tensor's device carries its index: compare what they resolve to"""
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return a.index == b.index
    cur = torch.cuda.current_device() if a.index is None or b.index is None else 0
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


def _per_utterance(lm_on, B):
    """lm_on of a decoding call: None, one value per utterance, or one value (bool / int) for all B of them"""
    if lm_on is None or torch.is_tensor(lm_on) or isinstance(lm_on, (list, tuple)):
        return lm_on
    return [lm_on] * B


class EndpointConfig:
    """The endpoint rule of a streaming decoder (include/m3asr.h, m3_ctc_endpoint_*).

    A frame whose argmax is the blank with probability above `blank_threshold` is a blank frame; any other frame ends the
    run of trailing blanks, and a frame whose argmax is a token means something has been decoded.  rules: up to four
    (must_decoded, min trailing blank ms, min utterance ms); after every frame the first rule that holds ends the utterance.
    The defaults: 5 s of silence before anything was said, 1 s of silence after something was said, or 20 s in all.
    Milliseconds become frames of `frame_ms` by ceil(ms / frame_ms).  blank_threshold lies in [0.5, 1): a blank above 0.5
    is the frame's argmax, so the detector needs nothing but the top-1 of the search's top-k."""

    def __init__(self, blank_threshold=0.8, rules=((False, 5000, 0), (True, 1000, 0), (False, 0, 20000)), frame_ms=40):
        self.blank_threshold, self.frame_ms = float(blank_threshold), int(frame_ms)
        if not 0.5 <= self.blank_threshold < 1.0:
            raise ValueError("EndpointConfig: blank_threshold = %r outside [0.5, 1)" % (blank_threshold,))
        if self.frame_ms <= 0:
            raise ValueError("EndpointConfig: frame_ms = %r" % (frame_ms,))
        self.rules = tuple((bool(m), t, n) for m, t, n in rules)
        if not 1 <= len(self.rules) <= 4:
            raise ValueError("EndpointConfig: %d rules, need 1 to 4" % len(self.rules))
        if any(t < 0 or n < 0 for _, t, n in self.rules):
            raise ValueError("EndpointConfig: negative time in %r" % (self.rules,))
        self.log_blank_threshold = float(np.float32(math.log(self.blank_threshold)))    # the float32 the kernel compares with
        self.frame_rules = tuple((m, self.frames(t), self.frames(n)) for m, t, n in self.rules)

    def frames(self, ms):
        """ceil(ms / frame_ms)"""
        return int(-(-ms // self.frame_ms)) if isinstance(ms, int) else int(math.ceil(ms / self.frame_ms))

    def length_bound(self):
        """Frames after which a rule fires whatever the audio holds (a rule without must_decoded and without trailing
        blanks), or None when no rule bounds an utterance's length."""
        return min((n for m, t, n in self.frame_rules if not m and t == 0), default=None)

    def desc(self, B, blank=0):
        return ops.ctc_endpoint_desc(B, blank, self.log_blank_threshold, self.frame_rules)


# what StreamingCtcDecoder.endpoints() returns per stream; rule == 0: no endpoint yet (frame is then -1)
EndpointInfo = collections.namedtuple("EndpointInfo", "rule frame frames trailing_blank decoded first_speech last_speech")


class CtcBeamSearch:
    """B prefix beam searches on the device, resumable at any frame boundary (m3_ctc_beam_*).

        search = CtcBeamSearch(B, beam, max_frames)
        search.advance(logits_chunk, n_frames)      # (B, Tc, V) device logits, (B,) frames of each row that count
        ...
        search.nbest()                              # [[(prefix tuple, score)], ...] per utterance, best first

    With context=ContextSet(...) the search is biased towards the set's phrase lists (m3asr.context), with lm=NgramLm(...)
    an n-gram LM is fused into the ranking (m3asr.lm): see __init__.

    The result equals the host routine (ops.ctc_prefix_beam_search_host) on each utterance's frames, however the frames are
    cut into chunks.  max_frames bounds the frames one utterance may consume between resets; past it nbest() raises."""

    def __init__(self, B, beam, max_frames, blank=0, device="cuda", k=None, context=None, lm=None, lm_weight=0.5,
                 length_bonus=0.0, lm_eos=True):
        """k: candidate symbols per frame (default beam, as the reference's logp.topk(beam_size)); needs k <= V.
        context: a m3asr.context.ContextSet uploaded to `device` -- the search then ranks by CTC score + bonus (hotword
        biasing, m3_ctc_beam_ctx_*).  Every utterance starts unbiased (graph -1); reset(graph_ids=) / set_context choose.
        lm: a m3asr.lm.NgramLm uploaded to `device` (lm.to(device)) -- the search then ranks a prefix y by
        (CTC score + bonus) + (lm_weight log P_LM(y) + length_bonus |y|) (shallow fusion, m3_ctc_beam_lm_*); lm_eos: the
        n-best is ordered with log P(</s> | y) added to the LM score.  Every utterance starts with the LM on; reset(lm_on=)
        switches it per utterance.  lm may also be a m3asr.lm.NgramLmSet (one device image of several LMs): reset(lm_on=)
        then picks a member per utterance, whose scale multiplies lm_weight; every utterance starts with member 0."""
        self.desc = ops.ctc_beam_desc(B, beam, max_frames, blank, k)
        self.device = torch.device(device)
        self.context = context
        self.lm, self.lm_weight, self.length_bonus, self.lm_eos = lm, float(lm_weight), float(length_bonus), bool(lm_eos)
        if context is not None and (context.dev is None or not _same_device(context.dev.device, self.device)):
            raise _lib.M3Error("CtcBeamSearch: the ContextSet is not on %s" % self.device)
        if lm is not None and (lm.dev is None or not _same_device(lm.dev.device, self.device)):
            raise _lib.M3Error("CtcBeamSearch: the NgramLm is not on %s (lm.to(device))" % self.device)
        self._bind_form()
        if not self._plain:
            self.graph_ids = [-1] * self.desc.B               # what each utterance's next reset installs
            self.graph_of = torch.full((max(self.desc.B, 1),), -1, dtype=torch.int32, device=self.device)[:self.desc.B]
            self.used = [False] * self.desc.B                 # advanced since its last reset
            self.lm_flags = [1] * self.desc.B
            self.lm_on = torch.ones(max(self.desc.B, 1), dtype=torch.int32, device=self.device)[:self.desc.B]
        self.state = torch.empty(max(self._size(self.desc), 1), dtype=torch.uint8, device=self.device)
        self.last_topk = None                                 # (top_logp, top_idx) of the last advance, for the endpointer
        self.reset()

    def _bind_form(self):
        """The form is decided once, here: the plain search (m3_ctc_beam_*), with a context and no LM the biased one
        (m3_ctc_beam_ctx_*), with an LM the fused one (m3_ctc_beam_lm_*, whose context image may be absent).  self._size, _reset,
        _advance, _nbest: the form's ops calls; self._args(): what its advance takes between the state and the frames, and its
        n-best behind the state (there followed by lm_eos), read from self when a call runs."""
        self._plain = self.context is None and self.lm is None
        ctx = lambda: (None if self.context is None else self.context.dev, self.graph_of)
        if self._plain:
            family, self._args = "ctc_beam_", lambda: ()
        elif self.lm is None:
            family, self._args = "ctc_beam_ctx_", ctx
        else:
            family, self._args = "ctc_beam_lm_", lambda: ctx() + (self.lm.dev, self.lm_on, self.lm_weight, self.length_bonus)
        self._size, self._reset, self._advance, self._nbest = (getattr(ops, family + op)
                                                               for op in ("state_size", "reset", "advance", "nbest"))

    @property
    def B(self):
        return self.desc.B

    @property
    def beam(self):
        return self.desc.beam

    def lm_weights(self):
        """The weight of log P_LM in each utterance's key: lm_weight, or with an NgramLmSet a (B, 1) float32 device tensor of
        lm_weight * scale of the utterance's member (an utterance without the LM has hyp_lm = 0, whatever stands here)."""
        if not isinstance(self.lm, _lm.NgramLmSet):
            return self.lm_weight
        w = [self.lm_weight * self.lm.scales[j - 1] if 1 <= j <= len(self.lm) else 0.0 for j in self.lm_flags]
        return torch.tensor(w, dtype=torch.float32).to(self.device).view(-1, 1)

    def set_context(self, slots, graph_ids):
        """Graph (position in the ContextSet, -1 = unbiased) of each listed utterance.  It takes effect at the utterance's
        next reset: a search keeps one graph from a reset to the next, because its nodes hold the context state and bonus
        of their prefixes.  Raises for an utterance that has consumed frames since its last reset -- restart it with
        reset(slots=, graph_ids=) instead."""
        if self.context is None:
            raise _lib.M3Error("CtcBeamSearch.set_context: the search was built without a context")
        slots, graph_ids = [int(b) for b in slots], [int(g) for g in graph_ids]
        if len(slots) != len(graph_ids):
            raise ValueError("set_context: %d slots, %d graph ids" % (len(slots), len(graph_ids)))
        for b, g in zip(slots, graph_ids):
            if not 0 <= b < self.B:
                raise ValueError("set_context: slot %d outside [0, %d)" % (b, self.B))
            if not -1 <= g < len(self.context):
                raise ValueError("set_context: graph %d outside [-1, %d)" % (g, len(self.context)))
            if self.used[b]:
                raise _lib.M3Error("set_context: utterance %d has consumed frames since its last reset" % b)
        for b, g in zip(slots, graph_ids):
            self.graph_ids[b] = g

    def reset(self, stream=None, slots=None, graph_ids=None, lm_on=None):
        """slots: None = all B searches; else the utterances to restart (a list, or an int32 device tensor).
        graph_ids (biased search): the graphs the restarted utterances take, one per slot (all B when slots is None).
        lm_on (fused search): whether each restarted utterance runs with the LM, one flag per slot; an utterance keeps its
        setting from a reset to the next, because its nodes hold the LM state and sum of their prefixes.  With an NgramLmSet
        the flags are ints: 0 / False = off, j = member j - 1 (True / 1 = member 0); a value above len(set) is refused.  A
        restarted utterance begins from its new member's start state."""
        if graph_ids is not None and self.context is None:
            raise _lib.M3Error("CtcBeamSearch.reset: graph_ids without a context")
        if lm_on is not None and self.lm is None:
            raise _lib.M3Error("CtcBeamSearch.reset: lm_on without an LM")
        if not self._plain:
            which = list(range(self.B)) if slots is None else [int(b) for b in (slots.tolist() if torch.is_tensor(slots) else slots)]
            which = [b for b in which if 0 <= b < self.B]
            for b in which:
                self.used[b] = False
            if graph_ids is not None:
                self.set_context(which, graph_ids)
            if lm_on is not None:
                if len(lm_on) != len(which):
                    raise ValueError("reset: %d slots, %d lm_on flags" % (len(which), len(lm_on)))
                for b, f in zip(which, _lm.lm_flags(self.lm, lm_on, len(which), "CtcBeamSearch.reset")):
                    self.lm_flags[b] = f
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.device)):
            if slots is not None and not torch.is_tensor(slots):
                slots = torch.tensor([int(b) for b in slots], dtype=torch.int32).to(self.device)
            if slots is None or slots.numel() > 0:
                self._reset(self.desc, self.state, slots)
                if self.lm is not None and self.B > 0:
                    self.lm_on.copy_(torch.tensor(self.lm_flags, dtype=torch.int32))
                if not self._plain and self.B > 0:
                    self.graph_of.copy_(torch.tensor(self.graph_ids, dtype=torch.int32))

    def advance(self, logits, n_frames, stream=None):
        """logits (B, Tc, V) on the device; n_frames (B,) how many of each row's Tc frames are real.  Enqueues m3_ctc_topk and
        the advance on `stream` (default: the current stream) without a host sync."""
        st = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            B, Tc, V = logits.shape
            assert B == self.B
            if Tc == 0:
                return
            nf = n_frames.reshape(-1).to(self.device, torch.int32, non_blocking=True)
            top_logp, top_idx = self.last_topk = ops.ctc_topk(logits.contiguous(), self.desc.k)
            assert self.context is None or V == self.context.vocab_size, "the ContextSet was built for another vocabulary size"
            assert self.lm is None or V == self.lm.vocab_size, "the NgramLm was built for another vocabulary size"
            if not self._plain:
                self.used = [True] * self.B               # without a sync the host cannot tell which rows had frames
            self._advance(self.desc, self.state, *self._args(), top_logp, top_idx, nf)

    def _nbest_tensors(self):
        """(hyp_tokens, hyp_len, hyp_score, hyp_bonus or None, hyp_lm or None, n_hyps): the plain form has no hyp_bonus, only the
        fused form a hyp_lm"""
        eos = () if self.lm is None else (self.lm_eos,)
        toks, hlen, score, *more, n = self._nbest(self.desc, self.state, *self._args(), *eos)
        bonus, lm = (more + [None, None])[:2]
        return toks, hlen, score, bonus, lm, n

    def nbest_tensors(self, stream=None, detail=False):
        """(hyp_tokens (B,beam,max_frames), hyp_len (B,beam), hyp_score (B,beam), n_hyps (B,)) on the device; detail: with
        hyp_bonus (B,beam) before n_hyps (zeros for a search without a context) and, for a search with an LM, hyp_lm (B,beam)
        after hyp_bonus."""
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.device)):
            toks, hlen, score, bonus, lm, n = self._nbest_tensors()
            if not detail:
                return toks, hlen, score, n
            bonus = torch.zeros_like(score) if bonus is None else bonus
            return (toks, hlen, score, bonus, n) if self.lm is None else (toks, hlen, score, bonus, lm, n)

    def nbest(self, stream=None, slots=None, detail=False):
        """slots: None = every utterance; else only the listed ones, in that order (the others may have failed or be idle).
        [(prefix, CTC score)] per utterance, best first -- with a context, best by CTC score + bonus, with an LM by the fused
        key; detail: [(prefix, CTC score, bonus)], bonus = the part of the context bonus that is final for that prefix, and
        for a search with an LM [(prefix, CTC score, bonus, lm)], lm = log P_LM(prefix) (+ log P(</s> | prefix) with lm_eos)."""
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.device)):   # the copies wait for the search's stream
            toks, hlen, score, bonus, lm, n = (None if t is None else t.cpu() for t in self._nbest_tensors())
        out = []
        for b in (range(self.B) if slots is None else [int(x) for x in slots]):
            nb = int(n[b])
            if nb < 0:
                raise _lib.M3Error("ctc beam search: utterance %d consumed more than max_frames = %d frames"
                                   % (b, self.desc.max_frames))
            hyps = [(tuple(toks[b, i, :int(hlen[b, i])].tolist()), float(score[b, i])) for i in range(nb)]
            if detail:
                hyps = [h + (0.0 if bonus is None else float(bonus[b, i]),) for i, h in enumerate(hyps)]
                if lm is not None:
                    hyps = [h + (float(lm[b, i]),) for i, h in enumerate(hyps)]
            out.append(hyps)
        return out


class CtcDecoder:
    """decoder = CtcDecoder(engine, blank_idx=0); engine: m3asr.engine.Engine (feat (B,T,idim), feat_len -> logits (B,T',V))."""

    def __init__(self, engine, blank_idx: int = 0, rescorer=None):
        """rescorer: a m3asr.rescore.AttentionRescorer on the engine's device, for attention_rescoring()."""
        self.engine = engine
        self.blank_idx = int(blank_idx)
        self.rescorer = rescorer

    def forward(self, xs: torch.Tensor, xs_lens: torch.Tensor):
        """-> {"out_nosm": logits (B,T',V) on the device, "out_lens": (B,) int32 on the device} (encoder.py:140-147)."""
        dev = self.engine.device
        feat = xs.to(dev, torch.float32).contiguous()
        lens = xs_lens.reshape(1, -1).to(dev, torch.int32).contiguous()
        logits = self.engine(feat, lens)
        out_lens = self.engine.buffer("lens", torch.int32)[:feat.shape[0]].clone()
        return {"out_nosm": logits, "out_lens": out_lens}

    def _full_context(self, decoding_chunk_size, num_decoding_left_chunks):
        # the engine computes one attention mask, fixed when it was built: the reference's "use full chunk" setting (< 0)
        # describes a full-context engine, a chunk size > 0 only an engine built with that static chunk mask
        assert decoding_chunk_size != 0, "decoding does not support dynamic chunks"
        if decoding_chunk_size > 0:
            cfg = getattr(self.engine, "cfg", None)
            chunk = int(getattr(cfg, "static_chunk_size", 0) or 0)
            left = int(getattr(cfg, "num_decoding_left_chunks", -1))
            if chunk <= 0:
                raise NotImplementedError("chunked decoding: the full-context encoder has no chunk mask")
            if decoding_chunk_size != chunk or num_decoding_left_chunks != left:
                raise NotImplementedError("chunked decoding: the engine was built for chunk %d / %d left chunks, asked for %d / %d"
                                          % (chunk, left, decoding_chunk_size, num_decoding_left_chunks))

    def ctc_greedy_search(self, xs: torch.Tensor, xs_lens: torch.Tensor, decoding_chunk_size: int = -1,
                          num_decoding_left_chunks: int = -1) -> List[List[int]]:
        self._full_context(decoding_chunk_size, num_decoding_left_chunks)
        res = self.forward(xs, xs_lens)
        return self.greedy_from_logits(res["out_nosm"], res["out_lens"])

    def greedy_from_logits(self, logits: torch.Tensor, out_lens: torch.Tensor) -> List[List[int]]:
        _, tokens, n_tokens = ops.ctc_greedy(logits, out_lens, self.blank_idx)
        tokens, n_tokens = tokens.cpu(), n_tokens.cpu().tolist()
        return [tokens[b, :n].tolist() for b, n in enumerate(n_tokens)]

    def ctc_prefix_beam_search(self, xs: torch.Tensor, xs_lens: torch.Tensor, beam_size: int,
                               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, return_hidden: bool = False
                               ) -> Tuple[List[Tuple[Tuple[int, ...], float]], torch.Tensor]:
        """-> (n-best [(prefix, ctc score)], logits (1,T',V)); batch size 1 as in the reference (encoder.py:213-214).
        return_hidden: the second item is the encoder's hidden states (1,T',D) (Engine.hidden()), which is what the reference
        returns there "for attention rescoring"; by default it stays the scores the search ran on, as callers of this
        method have come to expect."""
        assert xs.shape[0] == xs_lens.reshape(-1).shape[0] == 1, "prefix beam search supports batch size 1"
        self._full_context(decoding_chunk_size, num_decoding_left_chunks)
        res = self.forward(xs, xs_lens)
        hyps = self.prefix_beam_from_logits(res["out_nosm"], beam_size)
        return hyps, (self.engine.hidden() if return_hidden else res["out_nosm"])

    def prefix_beam_from_logits(self, logits: torch.Tensor, beam_size: int):
        """logits (1,T',V) or (T',V) on the device; all T' frames are searched (max_len, encoder.py:222)."""
        x = logits.reshape(-1, logits.shape[-1])
        top_logp, top_idx = ops.ctc_topk(x, beam_size)
        return ops.ctc_prefix_beam_search_host(top_logp.cpu().numpy(), top_idx.cpu().numpy(), beam_size, self.blank_idx)

    def batch_prefix_beam_search(self, xs: torch.Tensor, xs_lens: torch.Tensor, beam_size: int,
                                 decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1
                                 ) -> Tuple[List[List[Tuple[Tuple[int, ...], float]]], torch.Tensor]:
        """B utterances in one device search: -> ([n-best [(prefix, ctc score)] per utterance], logits (B,T',V))."""
        self._full_context(decoding_chunk_size, num_decoding_left_chunks)
        res = self.forward(xs, xs_lens)
        return self.batch_prefix_beam_from_logits(res["out_nosm"], res["out_lens"], beam_size), res["out_nosm"]

    def batch_prefix_beam_from_logits(self, logits: torch.Tensor, lens: torch.Tensor, beam_size: int, lm=None, lm_weight=0.5,
                                      length_bonus=0.0, lm_eos=True, context=None, graph_ids=None, lm_on=None):
        """logits (B,T',V) on the device, lens (B,) valid frames per utterance -> n-best per utterance (device search).
        lm: a m3asr.lm.NgramLm on the logits' device -- shallow fusion, as CtcBeamSearch(lm=).  context: a ContextSet on that
        device -- hotword biasing, as CtcBeamSearch(context=); graph_ids: one graph id per utterance (default graph 0 for all).
        lm_on: as CtcBeamSearch.reset takes it, one value per utterance, or one value for all of them (with an NgramLmSet as
        lm: 0 = off, j = member j - 1)."""
        B, T = int(logits.shape[0]), int(logits.shape[1])
        search = CtcBeamSearch(B, beam_size, T, self.blank_idx, logits.device, context=context, lm=lm, lm_weight=lm_weight,
                               length_bonus=length_bonus, lm_eos=lm_eos)
        if context is not None or lm_on is not None:
            search.reset(graph_ids=([0] * B if graph_ids is None else graph_ids) if context is not None else None,
                         lm_on=_per_utterance(lm_on, B))
        search.advance(logits, lens)
        return search.nbest()


    def ctc_wfst_search(self, xs: torch.Tensor, xs_lens: torch.Tensor, graph, decoding_chunk_size: int = -1,
                        num_decoding_left_chunks: int = -1, **kw):
        """WeNet's ctc_wfst_beam_search on the device: the forward, then token passing over `graph`, a m3asr.wfst.DecodingGraph
        on the engine's device.  -> word ids per utterance.  kw: CtcWfstSearch's options (beam, max_active, acoustic_scale,
        token_cap, record_cap, max_state_bytes, blank_skip: CTC blank-frame skipping with the decoder's blank id) and detail= (a
        dict per utterance: words, frames, cost, reached_final, status)."""
        self._full_context(decoding_chunk_size, num_decoding_left_chunks)
        res = self.forward(xs, xs_lens)
        return self.wfst_from_logits(res["out_nosm"], res["out_lens"], graph, **kw)

    def wfst_from_logits(self, logits: torch.Tensor, lens: torch.Tensor, graph, **kw):
        """logits (B,T',V) on the device, lens (B,) valid frames per utterance -> word ids per utterance (device search)."""
        from .wfst import wfst_from_logits
        if kw.get("blank_skip") is not None:
            kw.setdefault("blank", self.blank_idx)
        return wfst_from_logits(logits, lens, graph, **kw)

    def attention_rescoring(self, xs: torch.Tensor, xs_lens: torch.Tensor, beam_size: int, decoding_chunk_size: int = -1,
                            num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0, reverse_weight: float = 0.0,
                            context=None, graph_ids=None, lm=None, lm_weight=0.5, length_bonus=0.0, lm_eos=True, detail=False):
        """The reference's two-pass decoding (model/ctc_aed.py:160-252) for any batch size, all on the device: encoder
        forward, batched CTC prefix beam search, then the attention decoder rescoring each utterance's n-best on the
        encoder's hidden states (m3asr.rescore).  The prior that ctc_weight multiplies is the search's own ranking key: the
        CTC score, plus the context bonus and lm_weight log P_LM + length_bonus |y| when the search has them.
        -> the best token list per utterance; detail: AttentionRescorer.rescore's result, (best tokens, [(tokens, prior, att,
        final)]) per utterance."""
        if self.rescorer is None:
            raise _lib.M3Error("CtcDecoder.attention_rescoring: built without a rescorer (CtcDecoder(engine, rescorer=AttentionRescorer(...)))")
        self._full_context(decoding_chunk_size, num_decoding_left_chunks)
        res = self.forward(xs, xs_lens)
        return self.rescore_from_logits(res["out_nosm"], res["out_lens"], beam_size, ctc_weight=ctc_weight, reverse_weight=reverse_weight,
                                        context=context, graph_ids=graph_ids, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus,
                                        lm_eos=lm_eos, detail=detail)

    def rescore_from_logits(self, logits: torch.Tensor, lens: torch.Tensor, beam_size: int, ctc_weight: float = 0.0,
                            reverse_weight: float = 0.0, context=None, graph_ids=None, lm=None, lm_weight=0.5, length_bonus=0.0,
                            lm_eos=True, detail=False, lm_on=None):
        """attention_rescoring() behind the encoder: logits (B,T',V) and lens (B,) of the engine's LAST forward (its hidden states
        are read from the engine), however that forward was fed.  lm_on: as batch_prefix_beam_from_logits takes it."""
        if self.rescorer is None:
            raise _lib.M3Error("CtcDecoder.attention_rescoring: built without a rescorer (CtcDecoder(engine, rescorer=AttentionRescorer(...)))")
        search = CtcBeamSearch(int(logits.shape[0]), beam_size, int(logits.shape[1]), self.blank_idx, logits.device, context=context,
                               lm=lm, lm_weight=lm_weight, length_bonus=length_bonus, lm_eos=lm_eos)
        if graph_ids is not None or lm_on is not None:
            search.reset(graph_ids=graph_ids, lm_on=_per_utterance(lm_on, int(logits.shape[0])))
        search.advance(logits, lens)
        # the residual stream as it is: after_norm rides in the prologue of the rescorer's K / V GEMM
        out = self.rescorer.rescore(self.engine.hidden(normalized=False), lens, search, ctc_weight=ctc_weight,
                                    reverse_weight=reverse_weight, raw_memory=True)
        return out if detail else [list(best) for best, _ in out]

    def attention(self, xs: torch.Tensor, xs_lens: torch.Tensor, beam_size: int, decoding_chunk_size: int = -1,
                  num_decoding_left_chunks: int = -1, max_steps=None, detail=False, ctc_weight: float = 0.0, pre_beam=None,
                  lm=None, lm_weight: float = 0.0, length_bonus: float = 0.0, context=None, graph_ids=None, lm_on=None):
        """The reference's decoding mode `attention` for any batch size, all on the device: encoder forward, then the attention
        decoder's own autoregressive beam search over the encoder's hidden states (m3asr.aed_search).  There is
        no first pass, and the right-to-left decoder takes no part.  ctc_weight = 0: CTC scores take no part either.
        ctc_weight > 0: one-pass joint decoding: every candidate of every step is also scored by its CTC prefix
        probability on this forward's own logits and ranked by (1 - ctc_weight) att + ctc_weight ctc; pre_beam: candidates per
        hypothesis that reach the CTC scorer (default min(max(beam, ceil(1.5 beam)), 64, vocab)).  max_steps: the most tokens per hypothesis
        (default: the encoder's output frames, the reference's maxlen); it sizes the search's K / V cache.
        -> the best token list per utterance; detail: (best tokens, [(tokens, score, finished)]) per utterance, and
        (tokens, key, finished, att, ctc) per hypothesis in joint mode.
        lm: an NgramLm on the engine's device (NgramLm.to): n-gram LM fusion and a length bonus inside the search,
        the rank (1 - ctc_weight) att + ctc_weight ctc + lm_weight lm + length_bonus |y|; detail then appends lm to each hypothesis.
        context: a ContextSet on the engine's device: hotword biasing inside the search, the rank gains the
        hypothesis's bonus; graph_ids: one graph id per utterance (default graph 0 for all, -1 = unbiased); detail then appends
        bonus and final.  The context scores the pre-beam only: a hotword outside a row's pre_beam best is not rescued.
        lm_on: None or one value per utterance, as AttentionBeamSearch.search takes it: 0 / False = without the LM, and with an
        NgramLmSet as lm, j = member j - 1."""
        if self.rescorer is None:
            raise _lib.M3Error("CtcDecoder.attention: built without a rescorer (CtcDecoder(engine, rescorer=AttentionRescorer(...)))")
        self._full_context(decoding_chunk_size, num_decoding_left_chunks)
        res = self.forward(xs, xs_lens)
        return self.attention_from_logits(res["out_nosm"], res["out_lens"], beam_size, max_steps=max_steps, detail=detail,
                                          ctc_weight=ctc_weight, pre_beam=pre_beam, lm=lm, lm_weight=lm_weight,
                                          length_bonus=length_bonus, context=context, graph_ids=graph_ids, lm_on=lm_on)

    def attention_from_logits(self, logits: torch.Tensor, out_lens: torch.Tensor, beam_size: int, max_steps=None, detail=False,
                              ctc_weight: float = 0.0, pre_beam=None, lm=None, lm_weight: float = 0.0, length_bonus: float = 0.0,
                              context=None, graph_ids=None, lm_on=None):
        """attention() behind the encoder: logits (B,T',V) and out_lens (B,) of the engine's LAST forward (its hidden states are
        read from the engine), however that forward was fed."""
        if self.rescorer is None:
            raise _lib.M3Error("CtcDecoder.attention: built without a rescorer (CtcDecoder(engine, rescorer=AttentionRescorer(...)))")
        from .aed_search import AttentionBeamSearch
        res = {"out_nosm": logits, "out_lens": out_lens}
        memory = self.engine.hidden(normalized=False)     # after_norm rides in the prologue of the search's K / V GEMM
        B, frames = int(memory.shape[0]), int(memory.shape[1])
        steps = min(frames, self.rescorer.cfg.max_len - 1) if max_steps is None else int(max_steps)
        if steps < 1:
            raise _lib.M3Error("CtcDecoder.attention: max_steps = %d, need at least 1" % steps)
        # the searcher (state, K / V cache, work buffers) is kept across calls: sized by the step bound rounded up to a multiple
        # of 64 and re-allocated only when a call needs more; the call's own bound goes to search()
        key = (B, int(beam_size), float(ctc_weight), pre_beam, id(lm), float(lm_weight), float(length_bonus), id(context))
        kept = getattr(self, "_attention_search", None)
        if kept is None or kept[0] != key or kept[1].max_steps < steps:
            bound = min(-(-steps // 64) * 64, self.rescorer.cfg.max_len - 1)
            kept = self._attention_search = (key, AttentionBeamSearch(self.rescorer, B, beam_size, bound, ctc_weight=ctc_weight,
                                                                             pre_beam=pre_beam, lm=lm, lm_weight=lm_weight,
                                                                             length_bonus=length_bonus, context=context))
        ctc = res["out_nosm"][:, :frames] if float(ctc_weight) > 0 else None
        return kept[1].search(memory, res["out_lens"].cpu(), raw_memory=True, detail=detail, max_steps=steps, ctc_logits=ctc,
                              graph_ids=graph_ids, lm_on=_per_utterance(lm_on, B))

    def align(self, xs: torch.Tensor, xs_lens: torch.Tensor, tokens, frame_ms=40):
        """Encoder forward, then the best CTC alignment of tokens[b] to utterance b's frames (m3asr.align): one
        Alignment per utterance -- each token's start / end / peak frame and ms, its peak posterior, the alignment's score.  The
        token lists may come from any decoding mode of this class."""
        res = self.forward(xs, xs_lens)
        return self.align_from_logits(res["out_nosm"], res["out_lens"], tokens, frame_ms)

    def align_from_logits(self, logits: torch.Tensor, out_lens: torch.Tensor, tokens, frame_ms=40):
        """logits (B,T',V) on the device (scores or raw: the aligner normalises each frame itself), out_lens (B,) frames per
        utterance that count, tokens: one token list per utterance -> [Alignment] * B."""
        from .align import CtcAligner
        V = int(logits.shape[-1])
        kept = getattr(self, "_aligner", None)        # the aligner's workspace is reused while it suffices
        if kept is None or kept.V != V or kept.frame_ms != frame_ms or not _same_device(kept.device, logits.device):
            kept = self._aligner = CtcAligner(V, self.blank_idx, logits.device, frame_ms)
        return kept.align(logits, out_lens.cpu(), tokens)


class StreamingCtcDecoder:
    """CTC decoding chunk by chunk on top of a StreamingEncoder: every step() runs the chunk forward, then log-softmax +
    top-k, the prefix beam search advance and the streaming greedy search, all on the engine's stream; partial() reads the
    current best hypotheses, finish() the n-best.

        dec = StreamingCtcDecoder(engine.streaming(B, max_frames), beam=10)
        for n in range(n_chunks):
            dec.step(window_n, valid_n)
            best, greedy = dec.partial()
        nbest = dec.finish()

    The output frames of a chunk that count for a stream follow StreamingEncoder.decode: frames t < T'(len) of an utterance of
    len >= 7 feature frames.  step() derives them from `valid` (min(T'(valid), c), 0 for valid < 7); a caller that knows
    the utterance lengths passes them as n_out (decode() does).

    Over a slot-mode encoder (engine.streaming(..., independent=True)) the streams are independent here too: a slot that is
    idle in a step consumes no frame in either search, and reset / partial / finish take `slots=[...]`.

    With endpoint=EndpointConfig(...) every step() also advances the endpoint detector on the top-k the beam search just
    computed (one more small launch on the engine's stream, no second log-softmax, no sync); endpoints() tells which streams'
    utterances are over.

    With rescorer=AttentionRescorer(...) the decoder also keeps every stream's encoder memory: each step() appends the chunk's
    residual stream (the binding's buffer "x", before after_norm) to the stream's rows of a device store, with the same frame
    counts the beam search consumes (one more launch on the engine's stream, no sync, the chunk's graph is unchanged), and
    rescore() runs the attention decoder over the listed streams' current n-best.  The memory of a stream is exactly the
    frames its n-best was searched over.

    With aligner=CtcAligner(...) the decoder also keeps every stream's logits, in a second store of the same kind: each step()
    copies the chunk's (B c, V) logits into a (B c, Vp) buffer (Vp = V rounded up to a multiple of 4, what the store's 16-byte
    row copies need; the pad columns are never read) and appends it with the same frame counts, and align() gives the token
    times of a stream's hypothesis on exactly the frames it was searched over.

    With graph=DecodingGraph(...) the decoder also runs the WFST search (m3asr.wfst.CtcWfstSearch) over
    every stream: each step() advances it on the chunk's logits with the same frame counts the other searches consume (its
    launches on the engine's stream, no sync, the chunk's graph is unchanged), reset() restarts it with the slot, and words()
    reads each stream's word sequence.  The prefix beam search keeps running: the endpoint detector reads its top-k."""

    def __init__(self, streaming_encoder, beam, blank=0, context=None, lm=None, lm_weight=0.5, length_bonus=0.0, lm_eos=True,
                 endpoint=None, rescorer=None, ctc_weight=0.5, reverse_weight=0.0, aligner=None, graph=None, wfst=None):
        """context: a m3asr.context.ContextSet on the engine's device (hotword biasing of the beam search; the greedy
        search is not biased); reset(graph_ids=) chooses each stream's graph, -1 = unbiased.
        lm: a m3asr.lm.NgramLm on the engine's device (shallow fusion in the beam search, as CtcBeamSearch(lm=); the walk
        runs inside the advance kernel, so a chunk is still one graph replay and no host round trip); reset(lm_on=) switches
        it per stream.
        endpoint: an EndpointConfig; None = no endpoint detection (nothing is allocated for it, endpoints() raises).
        rescorer: a m3asr.rescore.AttentionRescorer on the engine's device for rescore(); ctc_weight / reverse_weight: the
        weights of the first pass and of the right-to-left decoder in its final score.  None = no second pass (nothing is
        allocated for it, step() launches nothing for it, rescore() raises).
        aligner: a m3asr.align.CtcAligner for the engine's vocabulary, blank and device, for align().  None = no token times
        (nothing is allocated for them, step() launches nothing for them, align() raises).
        graph: a m3asr.wfst.DecodingGraph on the engine's device for words(); wfst: a dict of CtcWfstSearch's options (beam,
        max_active, acoustic_scale, blank_skip, token_cap, record_cap, max_state_bytes); the search's B, max_frames and blank
        are the decoder's.  None = no graph search (nothing is allocated for it, step() launches nothing for it, words()
        raises)."""
        self.st = streaming_encoder
        self.graph, self.wfst = graph, None
        if wfst is not None and graph is None:            # refuse before anything is allocated or launched
            raise _lib.M3Error("StreamingCtcDecoder: wfst= options without graph=")
        if graph is not None:
            ecfg = streaming_encoder.eng.cfg
            if graph.vocab_size != ecfg.output_dim:
                raise _lib.M3Error("StreamingCtcDecoder: the graph was compiled for V = %d, the encoder's output_dim is %d"
                                   % (graph.vocab_size, ecfg.output_dim))
            if graph.dev is None:
                raise _lib.M3Error("StreamingCtcDecoder: the graph is not on a device (graph.to(device))")
            if not _same_device(graph.dev.device, streaming_encoder.eng.device):
                raise _lib.M3Error("StreamingCtcDecoder: the graph is on %s, the engine on %s" % (graph.dev.device, streaming_encoder.eng.device))
            known = ("beam", "max_active", "acoustic_scale", "blank_skip", "token_cap", "record_cap", "max_state_bytes")
            unknown = sorted(set(wfst or ()) - set(known))
            if unknown:
                raise _lib.M3Error("StreamingCtcDecoder: wfst= has unknown options %s (known: %s)" % (unknown, ", ".join(known)))
        self.aligner = aligner
        if aligner is not None:           # refuse before anything is allocated or launched
            ecfg = streaming_encoder.eng.cfg
            if aligner.V != ecfg.output_dim or aligner.blank != int(blank):
                raise _lib.M3Error("StreamingCtcDecoder: the aligner was built for V = %d / blank %d, the decoder has V = %d / blank %d"
                                   % (aligner.V, aligner.blank, ecfg.output_dim, int(blank)))
            if not _same_device(aligner.device, streaming_encoder.eng.device):
                raise _lib.M3Error("StreamingCtcDecoder: the aligner is on %s, the engine on %s" % (aligner.device, streaming_encoder.eng.device))
        self.rescorer, self.ctc_weight, self.reverse_weight = rescorer, float(ctc_weight), float(reverse_weight)
        if rescorer is not None:          # refuse before anything is allocated or launched
            ecfg = streaming_encoder.eng.cfg
            if rescorer.cfg.dim != ecfg.attention_dim or rescorer.cfg.vocab != ecfg.output_dim:
                raise _lib.M3Error("StreamingCtcDecoder: the rescorer's decoder has dim %d / vocab %d, the encoder attention_dim %d / "
                                   "output_dim %d" % (rescorer.cfg.dim, rescorer.cfg.vocab, ecfg.attention_dim, ecfg.output_dim))
            if not _same_device(rescorer.device, streaming_encoder.eng.device):
                raise _lib.M3Error("StreamingCtcDecoder: the rescorer is on %s, the engine on %s" % (rescorer.device, streaming_encoder.eng.device))
            if self.reverse_weight > 0 and rescorer.cfg.r_num_blocks == 0:
                raise _lib.M3Error("StreamingCtcDecoder: reverse_weight = %g needs a right-to-left decoder" % self.reverse_weight)
        self.context = context
        self.lm = lm
        e = streaming_encoder.eng
        self.c = streaming_encoder.c
        B, max_frames = int(streaming_encoder.desc.B), int(streaming_encoder.desc.max_frames)
        self.beam = CtcBeamSearch(B, beam, max_frames, blank, e.device, context=context, lm=lm, lm_weight=lm_weight,
                                  length_bonus=length_bonus, lm_eos=lm_eos)
        self.gdesc = ops.ctc_greedy_stream_desc(B, max_frames, blank)
        self.gstate = torch.empty(max(ops.ctc_greedy_stream_state_size(self.gdesc), 1), dtype=torch.uint8, device=e.device)
        self.frame_ids = torch.empty(B, self.c, dtype=torch.int32, device=e.device)
        self.n_out = torch.zeros(B, dtype=torch.int32, device=e.device)
        self.endpoint = endpoint
        if endpoint is not None:
            self.edesc = endpoint.desc(B, blank)
            self.estate = torch.empty(max(ops.ctc_endpoint_state_size(self.edesc), 1), dtype=torch.uint8, device=e.device)
            self.einfo = torch.empty(B, 8, dtype=torch.int32, device=e.device)
            self.einfo_host = torch.empty(B, 8, dtype=torch.int32, pin_memory=True)
        if rescorer is not None:
            self.mdesc = ops.aed_memory_desc(B, max_frames, e.cfg.attention_dim)
            self.mstate = torch.empty(max(ops.aed_memory_state_size(self.mdesc), 1), dtype=torch.uint8, device=e.device)
            self.mx = None                # the chunk binding's "x" as (B * c, D) rows, looked up after the first chunk
        if aligner is not None:
            vp = -(-aligner.V // 4) * 4
            self.ldesc = ops.aed_memory_desc(B, max_frames, vp)
            self.lstate = torch.empty(max(ops.aed_memory_state_size(self.ldesc), 1), dtype=torch.uint8, device=e.device)
            self.lrows = torch.zeros(B * self.c, vp, dtype=torch.float32, device=e.device)      # the chunk's logits, padded to Vp
        if graph is not None:
            from .wfst import CtcWfstSearch
            with torch.cuda.stream(e.stream):          # its constructor resets it: on the stream every later call uses
                self.wfst = CtcWfstSearch(graph, B, max_frames, blank=int(blank), **dict(wfst or {}))
        self.reset()

    def reset(self, slots=None, graph_ids=None, lm_on=None):
        """Restart all streams, or (slot-mode encoder) the listed slots: encoder state, beam search, greedy search,
        endpoint state, (decoder with a rescorer) the encoder memory and (decoder with an aligner) the kept logits.
        graph_ids (decoder with a context): the graph each restarted stream takes, one per slot; a stream restarted without
        one keeps the graph it had.  lm_on (decoder with an LM): whether each restarted stream runs with the LM; with an
        NgramLmSet an int per stream, 0 = off, j = member j - 1 (CtcBeamSearch.reset)."""
        kw = {} if lm_on is None else {"lm_on": lm_on}
        e = self.st.eng
        if slots is None:
            self.st.reset()
        else:
            self.st.reset(slots=slots)
        with torch.cuda.stream(e.stream):
            if slots is None:
                self.beam.reset(e.stream, graph_ids=graph_ids, **kw)
                ops.ctc_greedy_stream_reset(self.gdesc, self.gstate)
                if self.endpoint is not None:
                    ops.ctc_endpoint_reset(self.edesc, self.estate)
                if self.rescorer is not None:
                    ops.aed_memory_reset(self.mdesc, self.mstate)
                if self.aligner is not None:
                    ops.aed_memory_reset(self.ldesc, self.lstate)
                if self.wfst is not None:
                    self.wfst.reset()
            elif len(slots) > 0:
                lst = torch.tensor([int(b) for b in slots], dtype=torch.int32).to(e.device)
                # known inconsistency: a plain search restarted by slots is not shown lm_on, so it does not refuse it
                self.beam.reset(e.stream, slots=[int(b) for b in slots], graph_ids=graph_ids,
                                **({} if self.context is None and self.lm is None else kw))
                ops.ctc_greedy_stream_reset(self.gdesc, self.gstate, lst)
                if self.endpoint is not None:
                    ops.ctc_endpoint_reset(self.edesc, self.estate, lst)
                if self.rescorer is not None:
                    ops.aed_memory_reset(self.mdesc, self.mstate, lst)
                if self.aligner is not None:
                    ops.aed_memory_reset(self.ldesc, self.lstate, lst)
                if self.wfst is not None:
                    self.wfst.reset(lst)

    def frames_of(self, valid):
        """Output frames of this chunk that count, from the real feature frames in its window."""
        v = torch.as_tensor(valid).reshape(-1).to("cpu", torch.int64)
        return torch.tensor([min(subsampled_len(int(x)), self.c) if x >= 7 else 0 for x in v], dtype=torch.int32)

    def step(self, window, valid, n_out=None, use_graph=True):
        """One chunk: window (B, 4c+3, idim), valid (B,) as for StreamingEncoder.step; n_out (B,) output frames of this chunk
        that count (default: frames_of(valid)).  Returns the chunk's logits buffer (B, c, V)."""
        e = self.st.eng
        if n_out is None:
            n_out = self.frames_of(valid)
        logits = self.st.step(window, valid, use_graph=use_graph)
        with torch.cuda.stream(e.stream):
            self.n_out.copy_(torch.as_tensor(n_out).reshape(-1).to(torch.int32), non_blocking=True)
            self.beam.advance(logits, self.n_out, e.stream)
            ops.ctc_greedy_stream_advance(self.gdesc, self.gstate, logits, self.n_out, self.frame_ids)
            if self.endpoint is not None:
                top_logp, top_idx = self.beam.last_topk
                ops.ctc_endpoint_advance(self.edesc, self.estate, top_logp, top_idx, self.n_out)
            if self.rescorer is not None:
                if self.mx is None:
                    self.mx = self.st.buffer("x").view(-1, self.mdesc.D)
                ops.aed_memory_append(self.mdesc, self.mstate, self.mx, self.n_out)
            if self.aligner is not None:
                self.lrows[:, :self.aligner.V].copy_(logits.reshape(-1, self.aligner.V))
                ops.aed_memory_append(self.ldesc, self.lstate, self.lrows, self.n_out)
            if self.wfst is not None:
                self.wfst.advance(logits, self.n_out)
        return logits

    def words(self, slots=None, final=False, detail=False):
        """Decoder with a graph: the word ids of every stream's best token after the chunks so far (slots: only the listed
        streams, in that order), with the meaning of CtcWfstSearch.result -- final: the graph's final weights count; detail:
        a dict per stream with words, frames (output frames counted from the stream's last reset, real ones with blank_skip
        too), cost, reached_final and status.  Raises M3Error for a listed stream that overflowed a capacity.  The streams go
        on as they were.  Waits for the engine's stream."""
        if self.wfst is None:
            raise _lib.M3Error("StreamingCtcDecoder.words: the decoder was built without a graph "
                               "(StreamingCtcDecoder(..., graph=DecodingGraph(...)))")
        B = self.wfst.B
        which = list(range(B)) if slots is None else [int(b) for b in slots]
        if any(not 0 <= b < B for b in which):
            raise ValueError("StreamingCtcDecoder.words: slots %s outside [0, %d)" % (which, B))
        if not which:
            return []
        with torch.cuda.stream(self.st.eng.stream):
            return self.wfst.result(final=final, detail=detail, slots=which)

    def decode_words(self, feat, feat_len, use_graph=True):
        """Whole utterances chunk by chunk, as decode() -> words(final=True)."""
        if self.wfst is None:
            raise _lib.M3Error("StreamingCtcDecoder.decode_words: the decoder was built without a graph "
                               "(StreamingCtcDecoder(..., graph=DecodingGraph(...)))")
        self.decode(feat, feat_len, use_graph)
        return self.words(final=True)

    def align(self, slots=None, tokens=None):
        """Token times of the streams' hypotheses on the frames they were searched over (slots: only the listed streams, in
        that order; tokens: one token list per listed stream, default each stream's current best beam hypothesis): one
        m3asr.align.Alignment per stream, None for a stream that ran past max_frames.  The kept logits are gathered (one
        launch) and aligned (two).  The streams go on as they were.  Waits for the engine's stream."""
        if self.aligner is None:
            raise _lib.M3Error("StreamingCtcDecoder.align: the decoder was built without an aligner "
                               "(StreamingCtcDecoder(..., aligner=CtcAligner(...)))")
        e = self.st.eng
        which = list(range(self.ldesc.B)) if slots is None else [int(b) for b in slots]
        if any(not 0 <= b < self.ldesc.B for b in which):
            raise ValueError("StreamingCtcDecoder.align: slots %s outside [0, %d)" % (which, self.ldesc.B))
        if tokens is not None and len(tokens) != len(which):
            raise ValueError("StreamingCtcDecoder.align: %d streams, %d token lists" % (len(which), len(tokens)))
        if not which:
            return []
        with torch.cuda.stream(e.stream):
            held = ops.aed_memory_lengths(self.ldesc, self.lstate).cpu().tolist()
            lst = torch.tensor(which, dtype=torch.int32).to(e.device)
            rows, row0 = ops.aed_memory_gather(self.ldesc, self.lstate, lst)
            row0 = row0.cpu().tolist()
            good = [j for j, b in enumerate(which) if held[b] >= 0]
            if tokens is None:
                best = self.beam.nbest(e.stream, slots=[which[j] for j in good])
                tokens = [None] * len(which)
                for j, hyps in zip(good, best):
                    tokens[j] = list(hyps[0][0]) if hyps else []
            out = [None] * len(which)
            if good:
                res = self.aligner.align_rows(rows[:, :self.aligner.V], [row0[j] for j in good], [row0[j + 1] - row0[j] for j in good],
                                              [tokens[j] for j in good])
                for j, a in zip(good, res):
                    out[j] = a
        return out

    def memory_lengths(self):
        """Decoder with a rescorer: encoder-memory frames every stream holds, (B,) int32 on the host; -1 for a stream that
        ran past max_frames.  Waits for the engine's stream."""
        if self.rescorer is None:
            raise _lib.M3Error("StreamingCtcDecoder.memory_lengths: the decoder was built without a rescorer")
        e = self.st.eng
        with torch.cuda.stream(e.stream):
            n = ops.aed_memory_lengths(self.mdesc, self.mstate)
        e.stream.synchronize()
        return n.cpu()

    def memory(self, slots=None):
        """Decoder with a rescorer: (rows (R, D), row0 (n + 1,) int32) on the device -- the listed streams' encoder memory
        packed in list order (the residual stream before after_norm), as m3_aed_memory_gather leaves it; stream j of the
        list owns rows [row0[j], row0[j + 1]).  Enqueued on the engine's stream."""
        if self.rescorer is None:
            raise _lib.M3Error("StreamingCtcDecoder.memory: the decoder was built without a rescorer")
        e = self.st.eng
        which = list(range(self.mdesc.B)) if slots is None else [int(b) for b in slots]
        with torch.cuda.stream(e.stream):
            lst = torch.tensor(which, dtype=torch.int32).to(e.device)
            return ops.aed_memory_gather(self.mdesc, self.mstate, lst)

    def rescore(self, slots=None, detail=False):
        """The second pass over the streams' current n-best (slots: only the listed streams, in that order): their encoder
        memory is gathered (one launch), the attention decoder scores every hypothesis teacher-forced and picks per stream
        (m3asr.rescore; final = (1 - reverse_weight) att + reverse_weight r_att + ctc_weight prior, the prior being the
        search's own ranking key).  -> the best token list per stream; detail: AttentionRescorer.rescore's pair per stream,
        (best tokens, [(tokens, prior, att, final)] in n-best order).  A stream that has consumed no frame gives ((), []).
        The streams go on as they were: call it before reset() when an utterance ends.  Waits for the engine's stream."""
        if self.rescorer is None:
            raise _lib.M3Error("StreamingCtcDecoder.rescore: the decoder was built without a rescorer "
                               "(StreamingCtcDecoder(..., rescorer=AttentionRescorer(...)))")
        e = self.st.eng
        which = list(range(self.mdesc.B)) if slots is None else [int(b) for b in slots]
        if any(not 0 <= b < self.mdesc.B for b in which):
            raise ValueError("StreamingCtcDecoder.rescore: slots %s outside [0, %d)" % (which, self.mdesc.B))
        if not which:
            return []
        rows, row0 = self.memory(which)
        with torch.cuda.stream(e.stream):
            out = self.rescorer.rescore_rows(rows, row0, self.beam, streams=which, ctc_weight=self.ctc_weight,
                                             reverse_weight=self.reverse_weight, raw_memory=True)
        return out if detail else [list(best) for best, _ in out]

    def endpoints(self, slots=None):
        """One EndpointInfo per stream (slots: only the listed streams, in that order) after the chunks so far; rule != 0:
        that rule ended the stream's utterance at output frame `frame` (counted from the stream's last reset), and the
        detector stands still until the stream is reset.  Waits for the engine's stream."""
        if self.endpoint is None:
            raise _lib.M3Error("StreamingCtcDecoder.endpoints: the decoder was built without an endpoint config")
        e = self.st.eng
        with torch.cuda.stream(e.stream):
            ops.ctc_endpoint_read(self.edesc, self.estate, self.einfo)
            self.einfo_host.copy_(self.einfo, non_blocking=True)
        e.stream.synchronize()
        rows = self.einfo_host.tolist()
        return [EndpointInfo(r[5], r[6], r[0], r[1], bool(r[2]), r[3], r[4])
                for r in (rows[int(b)] for b in (range(len(rows)) if slots is None else slots))]

    def greedy(self, slots=None):
        """Greedy hypotheses of the frames so far: [[token, ...]] per stream (slots: only the listed streams)."""
        e = self.st.eng
        with torch.cuda.stream(e.stream):
            toks, n = ops.ctc_greedy_stream_tokens(self.gdesc, self.gstate)
        e.stream.synchronize()
        toks, n = toks.cpu(), n.cpu().tolist()
        which = list(range(len(n))) if slots is None else [int(b) for b in slots]
        if min((n[b] for b in which), default=0) < 0:
            raise _lib.M3Error("streaming greedy search: a stream ran past max_frames")
        return [toks[b, :n[b]].tolist() for b in which]

    def partial(self, slots=None):
        """(best prefix beam hypothesis (prefix, score) per stream, greedy tokens per stream) after the chunks so far."""
        e = self.st.eng
        nb = self.beam.nbest(e.stream, slots=slots)
        return [h[0] for h in nb], self.greedy(slots)

    def finish(self, slots=None, detail=False):
        """n-best [(prefix, score)] per stream, best first (slots: only the listed streams, in that order); detail:
        [(prefix, CTC score, bonus)] as CtcBeamSearch.nbest."""
        return self.beam.nbest(self.st.eng.stream, slots=slots, detail=detail)

    def decode(self, feat, feat_len, use_graph=True):
        """Whole utterances chunk by chunk (the windows and frame counts of StreamingEncoder.decode) -> finish()."""
        c, st = self.c, self.st
        B, T = int(feat.shape[0]), int(feat.shape[1])
        lens = feat_len.reshape(-1).to("cpu", torch.int64)
        n_chunks = -(-subsampled_len(T) // c)
        total = torch.tensor([subsampled_len(int(v)) if v >= 7 else 0 for v in lens], dtype=torch.int64)
        self.reset()
        st.eng.stream.wait_stream(torch.cuda.current_stream())
        padded = torch.zeros(B, max(T, 4 * c * n_chunks + 3), feat.shape[2], dtype=torch.float32, device=st.eng.device)
        padded[:, :T] = feat.to(st.eng.device)
        for n in range(n_chunks):
            left = (lens - 4 * c * n).clamp(min=0, max=st.window)
            left = torch.where(left >= 7, left, torch.zeros_like(left))
            self.step(padded[:, 4 * c * n: 4 * c * n + st.window], left, (total - n * c).clamp(min=0, max=c), use_graph)
        return self.finish()
