"""Attention decoding on the device: the AED decoder searching on its own, autoregressively, with a beam (the reference's
decoding mode `attention`; the per-step decoder is layer/att_decoder.py:258-299 forward_one_step, a bidirectional decoder
searches with its left decoder only, att_decoder.py:389-411; the step's two helpers are utils/mask.py:205-251).  The contract
is restated in tests/aed_search_ref.py; DESIGN.md 21 has the design.

    rescorer = AttentionRescorer(packed, decoder_config_of(extra), device)        # the uploaded decoder weights
    search = AttentionBeamSearch(rescorer, B, beam, max_steps)
    best = search.search(engine.hidden(), out_lens)                               # a token list per utterance

R = B * beam hypothesis rows take one new token per step.  A step is ALWAYS the same launches with the same arguments --
m3_aed_search_embed, per block eight launches (fused QKV GEMM with the norm1 prologue, self-attention over the K / V cache,
linear_out with the residual, the source attention's Q GEMM with norm2, source attention over the memory's K / V projection,
linear_out with the residual, the two FFN GEMMs), the output layer with after_norm, m3_aed_search_prune: 8 L + 3 -- because the
position, who is finished and which utterance is done live in the device state.  The host enqueues steps without
synchronising and reads the B done flags in one small copy every `poll` steps; steps issued past an utterance's end are
no-ops for it.  The (R, V) log-probabilities never leave the device.  There is no torch fallback.

Memory: the self-attention K / V cache holds num_blocks * max_steps * B * beam * 2 * dim floats (6 blocks, 125 steps, 16 x 10
rows, dim 512: 0.49 GB) -- it is sized from max_steps, so give the constructor the bound you need, not the table's length.

JOINT CTC/ATTENTION DECODING (ctc_weight > 0; the contract is restated in tests/aed_joint_ref.py).  Every step
also scores its candidates with the CTC prefix probability and ranks them by (1 - ctc_weight) att + ctc_weight ctc: a row
offers its `pre_beam` largest attention log-probabilities, m3_aed_joint_score runs every candidate's prefix recursion over the
utterance's CTC log-probabilities, m3_aed_joint_prune keeps the `beam` best keys and moves the scorer states with the
hypotheses.  Those two launches stand where m3_aed_search_prune stood: 8 L + 4.  The CTC output comes with the call
(ctc_logits / ctc_rows, one row per memory row); its log-softmax runs on the device once per call.  With ctc_weight = 0 nothing
of this exists: no scorer state, the same launches, the same bits as before.

N-GRAM LM FUSION AND A LENGTH BONUS (lm=; the contract is restated in tests/aed_lm_ref.py).  With an NgramLm
(m3asr.lm, already moved with .to(device)) every candidate also takes one step through the LM and the rank is
(1 - ctc_weight) att + ctc_weight ctc + lm_weight lm + length_bonus n, n the hypothesis's tokens, eos included.
m3_aed_ngram_score and m3_aed_ngram_prune stand where the joint calls stood: still 8 L + 4.  ctc_weight = 0 with an LM is attention
plus LM: no CTC input, no scorer state; the rows still offer `pre_beam` candidates, because the LM scores the pre-beam only.
lm_on (per call, per utterance) switches the LM off for single utterances, which then get the bits of the search without it.
With an NgramLmSet lm_on holds ints: 0 = off, j = member j - 1, whose scale multiplies lm_weight; an utterance gets
the bits of the search with that member alone and lm_weight * scale.
Without lm nothing of this exists.

HOTWORD BIASING (context=; the contract is restated in tests/aed_ctx_ref.py).  With a ContextSet (m3asr.context,
built with device=) every candidate also takes one arc of its utterance's context graph and the rank gains the hypothesis's
bonus: key = jkey + (float)((lm_weight lm + length_bonus n) + bonus), the parenthesis without an LM being bonus alone.  The
graph's own score is the weight.  A token adds delta[state][cls[token]], eos hands back pot[state] (the credit of a phrase that
was not completed), so a finished hypothesis's bonus is the context contract's `final`; a hypothesis cut at the step limit
keeps its provisional credit and detail reports final = bonus - pot[state] next to it.  graph_ids (per call, per utterance)
picks the graph: default graph 0 for all, -1 = unbiased, and an unbiased utterance gets the bits of the search without a
context.  m3_aed_bias_score and m3_aed_bias_prune stand where the joint / ngram calls stood: still 8 L + 4, also with ctc_weight
= 0 and no LM.  The context is a PARTIAL scorer over the pre-beam, like the LM: the rows offer `pre_beam` candidates whenever a
context is given, whatever ctc_weight and lm are, and a hotword token outside a row's `pre_beam` largest attention
log-probabilities is not rescued.  A set in which eos is part of a phrase is refused: eos is never walked.  Without context
nothing of this exists."""
import math

import torch

from . import _lib, ops
from .lm import NgramLmSet, lm_flags
from .rescore import LN_EPS


class AttentionBeamSearch:
    def __init__(self, rescorer, B, beam, max_steps, poll=8, use_graph=False, ctc_weight=0.0, pre_beam=None, lm=None, lm_weight=0.0,
                 length_bonus=0.0, lm_eos=True, context=None):
        """rescorer: the AttentionRescorer whose uploaded weights and config the search shares; B utterances per call, `beam`
        hypotheses each (1 <= beam <= min(64, vocab)); max_steps: the most tokens a hypothesis can get (it sizes the state and
        the K / V cache, see the module docstring; more than max_len - 1 steps are never taken).  poll: steps between two reads of
        the done flags.  use_graph: capture the step once with torch.cuda.graph and replay it (the step is a straight line of
        launches whose arguments never change); off by default: the A/B in DESIGN.md 21 shows no gain.  The first graph call
        of an object pays one extra eager step, a synchronisation and the capture.
        ctc_weight in [0, 1]: above 0 the search is the joint CTC/attention search (module docstring) and every call must bring
        the CTC output; pre_beam: the candidates a row offers to the CTC scorer, beam <= pre_beam <= min(64, vocab), default
        min(max(beam, ceil(1.5 beam)), 64, vocab).  The scorer state is allocated by the first call, from its longest memory.
        lm: an NgramLm over the decoder's vocabulary, already moved with .to(device) (which validates it); lm_weight and
        length_bonus: the weights of its log-probability and of the token count in the key; lm_eos: a hypothesis that ends also
        takes log P(</s> | its LM state).  pre_beam applies whenever lm is given, whatever ctc_weight.
        context: a ContextSet over the decoder's vocabulary, built with device= this search's device (its constructor validates
        it); the phrases' score is the weight of the bonus in the key.  pre_beam applies whenever context is given, whatever
        ctc_weight and lm: the context scores the pre-beam only, a hotword outside a row's pre_beam best is not rescued.  A set
        on the host, on another device, over another vocabulary, or with eos in a phrase is refused.
        Raises M3Error before anything is allocated for a beam or a head size the kernels do not take."""
        cfg = rescorer.cfg
        self.rescorer, self.cfg, self.device = rescorer, cfg, rescorer.device
        self.B, self.beam, self.poll, self.use_graph = int(B), int(beam), max(int(poll), 1), bool(use_graph)
        if self.beam < 1 or self.beam > cfg.vocab or self.beam > 64:
            raise _lib.M3Error("AttentionBeamSearch: beam = %d, need 1 <= beam <= min(64, vocab = %d)" % (self.beam, cfg.vocab))
        if int(max_steps) < 1:
            raise _lib.M3Error("AttentionBeamSearch: max_steps = %d, need at least 1" % int(max_steps))
        self.ctc_weight = float(ctc_weight)
        if not 0.0 <= self.ctc_weight <= 1.0:                      # also refuses NaN
            raise _lib.M3Error("AttentionBeamSearch: ctc_weight = %r outside [0, 1]" % (ctc_weight,))
        self.lm, self.lm_weight, self.length_bonus, self.lm_eos = lm, float(lm_weight), float(length_bonus), bool(lm_eos)
        if lm is not None:
            if not (math.isfinite(self.lm_weight) and math.isfinite(self.length_bonus)):
                raise _lib.M3Error("AttentionBeamSearch: lm_weight = %r / length_bonus = %r is not finite" % (lm_weight, length_bonus))
            if lm.dev is None or not lm.dev.is_cuda:
                raise _lib.M3Error("AttentionBeamSearch: the LM is not on %s; move it with NgramLm.to(device), which validates it" % (self.device,))
            if lm.vocab_size != cfg.vocab:
                raise _lib.M3Error("AttentionBeamSearch: the LM was built for a vocabulary of %d, the attention decoder has %d" % (
                    lm.vocab_size, cfg.vocab))
        self.context = context
        if context is not None:
            if context.dev is None or not context.dev.is_cuda or context.dev.device != torch.device(self.device):
                raise _lib.M3Error("AttentionBeamSearch: the context set is not on %s; build it with ContextSet(graphs, device=...)" % (
                    self.device,))
            if context.vocab_size != cfg.vocab:
                raise _lib.M3Error("AttentionBeamSearch: the context set was built for a vocabulary of %d, the attention decoder has %d" % (
                    context.vocab_size, cfg.vocab))
            for i, g in enumerate(context.graphs):
                if int(g.cls[cfg.vocab - 1]) != 0:
                    raise _lib.M3Error("AttentionBeamSearch: graph %d of the context set has eos (%d) in a phrase; eos is never walked" % (
                        i, cfg.vocab - 1))
        self.pre_beam = 0
        if self.ctc_weight > 0 or lm is not None or context is not None:
            self.pre_beam = min(max(self.beam, math.ceil(1.5 * self.beam)), 64, cfg.vocab) if pre_beam is None else int(pre_beam)
            if not self.beam <= self.pre_beam <= min(64, cfg.vocab):
                raise _lib.M3Error("AttentionBeamSearch: pre_beam = %d, need beam = %d <= pre_beam <= min(64, vocab = %d)" % (
                    self.pre_beam, self.beam, cfg.vocab))
            if cfg.vocab < 2:
                raise _lib.M3Error("AttentionBeamSearch: joint decoding needs blank and eos to be two ids, vocab = %d" % cfg.vocab)
        self.max_steps = min(int(max_steps), cfg.max_len - 1)
        self.desc = ops.aed_search_desc(self.B, self.beam, self.max_steps, cfg.vocab, cfg.dim, cfg.heads, cfg.num_blocks, cfg.max_len)
        R, D, dev = self.B * self.beam, cfg.dim, self.device
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)   # noqa: E731
        self.state = torch.zeros(ops.aed_search_state_size(self.desc), dtype=torch.uint8, device=dev)
        self.cache = torch.zeros(ops.aed_search_cache_size(self.desc) // 4, dtype=torch.float32, device=dev)
        # zeros, not empty: the rows of a done utterance are skipped by the kernels and the GEMMs still read them
        self.x, self.qkv, self.ctx, self.q = f32(R, D), f32(R, 3 * D), f32(R, D), f32(R, D)
        self.h, self.logits = f32(R, cfg.linear_units), f32(R, cfg.vocab)
        self.done = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._done_host = torch.zeros(self.B, dtype=torch.int32).pin_memory()     # the poll's target: one small asynchronous copy
        # joint decoding only: descriptor, scorer state and candidate scratch, sized by the first call that needs them
        self.jdesc = self.jstate = self.jscratch = self.ctc = None
        # LM fusion only: its descriptor without a CTC part, the LM state and scratch (sized by B, beam and pre_beam alone), lm_on
        self.ldesc = self.lstate = self.lscratch = self.lm_on = None
        if lm is not None:
            self.ldesc = ops.aed_lm_desc(self.desc, self.pre_beam)
            self.lstate = torch.zeros(ops.aed_lm_state_size(self.ldesc), dtype=torch.uint8, device=dev)
            self.lscratch = torch.zeros(ops.aed_lm_scratch_size(self.ldesc), dtype=torch.uint8, device=dev)
            self.lm_on = torch.ones(self.B, dtype=torch.int32, device=dev)
        # hotword biasing only: its descriptor without a CTC part, the context state and scratch (sized by B, beam and pre_beam
        # alone), graph_of, and the m3_aed_bias record that names them (the same addresses for every step and every call)
        self.bdesc = self.cstate = self.cscratch = self.graph_of = self.bias = None
        if context is not None:
            self.bdesc = ops.aed_bias_desc(self.desc, self.pre_beam)
            self.cstate = torch.zeros(ops.aed_bias_state_size(self.bdesc), dtype=torch.uint8, device=dev)
            self.cscratch = torch.zeros(ops.aed_bias_scratch_size(self.bdesc), dtype=torch.uint8, device=dev)
            self.graph_of = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.bias = ops.aed_bias_record(context.dev, self.graph_of, self.cstate, self.cscratch)
        self.kvp = None          # the memory's K / V projection of the current call, (rows, num_blocks * 2 D)
        self._graph = None
        self.steps_issued = 0     # of the last call
        self.last = None          # device tensors of the last call: m3_aed_search_result's, plus state and done
        self._bind_form()

    def _bind_form(self):
        """The form of the search, decided once; every call reads self when it runs: _take_ctc replaces jdesc and the
        scorer blobs, lm_weight and length_bonus are launch arguments.  self._tail: a step's calls behind the output layer: without
        CTC, LM and context m3_aed_search_prune, else the score and prune of the family that takes every part present, on jdesc
        with CTC, else on the context's or the LM's descriptor.  self._parts: the parts present in the order joint, LM, context,
        each (reset call, result call, the result's key of its att part, the floats it alone adds to detail)."""
        ctc, lm, ctx = self.ctc_weight > 0, self.lm is not None, self.context is not None
        blobs = lambda: (self.jdesc if ctc else self.bdesc if ctx else self.ldesc, self.state, self.jstate, self.jscratch,   # noqa: E731
                         self.lstate, self.lscratch)
        inputs = lambda: (self.logits, self.ctc, self.ctc_weight) + (   # noqa: E731
            (self.lm.dev, self.lm_on, self.lm_weight, self.length_bonus) if lm else (None, None, 0.0, 0.0)) + (self.lm_eos,)
        if ctx:
            self._tail = [lambda: ops.aed_bias_score(*blobs(), *inputs(), self.bias), lambda: ops.aed_bias_prune(*blobs(), self.bias, self.done)]
        elif lm:
            self._tail = [lambda: ops.aed_lm_score(*blobs(), *inputs()), lambda: ops.aed_lm_prune(*blobs(), self.done)]
        elif ctc:                                                  # the joint family takes neither the LM blobs nor the LM inputs
            self._tail = [lambda: ops.aed_joint_score(*blobs()[:4], *inputs()[:3]), lambda: ops.aed_joint_prune(*blobs()[:4], self.done)]
        else:
            self._tail = [lambda: ops.aed_search_prune(self.desc, self.state, self.logits, self.done)]
        self._parts = []
        if ctc:
            self._parts.append((lambda: ops.aed_joint_reset(self.jdesc, self.state, self.jstate, self.ctc),
                                lambda: dict(ops.aed_joint_result(self.jdesc, self.state, self.jstate), joint_state=self.jstate), "att", []))
        if lm:                                                    # a set: every utterance starts in its own member's start state
            lm_reset = ((lambda: ops.aed_lm_reset_set(self.ldesc, self.lstate, self.lm.dev, self.lm_on)) if isinstance(self.lm, NgramLmSet)
                        else (lambda: ops.aed_lm_reset(self.ldesc, self.lstate, self.lm.dev)))
            self._parts.append((lm_reset, lambda: dict(ops.aed_lm_result(self.ldesc, self.state, self.lstate), lm_blob=self.lstate), "lm_att", ["lm"]))
        if ctx:
            self._parts.append((lambda: ops.aed_bias_reset(self.bdesc, self.bias),
                                lambda: dict(ops.aed_bias_result(self.bdesc, self.state, self.bias), ctx_blob=self.cstate), "ctx_att", ["bonus"]))

    def launches_per_step(self):
        return 8 * self.cfg.num_blocks + 2 + len(self._tail)

    # ---- one step: the same launches with the same arguments, whatever the step
    def _step(self):
        w, cfg, d, st = self.rescorer.w, self.cfg, self.desc, self.state
        D, x = cfg.dim, self.x
        ops.aed_search_embed(d, st, w["decoder.embed.weight"], w["decoder.pe"], x)
        for i in range(cfg.num_blocks):
            q = "decoder.layers.%d." % i
            ln = lambda n: (w[q + n + ".weight"], w[q + n + ".bias"], LN_EPS)   # noqa: E731
            ops.linear(x, w[q + "self_attn.qkv.weight"], w[q + "self_attn.qkv.bias"], ln=ln("norm1"), out=self.qkv)
            ops.aed_search_attention(d, st, self.qkv[:, :D], self.qkv[:, D:], self.ctx, i, cache=self.cache)
            ops.linear(self.ctx, w[q + "self_attn.linear_out.weight"], w[q + "self_attn.linear_out.bias"], resid=x, out=x)
            ops.linear(x, w[q + "src_attn.linear_q.weight"], w[q + "src_attn.linear_q.bias"], ln=ln("norm2"), out=self.q)
            ops.aed_search_attention(d, st, self.q, self.kvp[:, i * 2 * D:(i + 1) * 2 * D], self.ctx, i)
            ops.linear(self.ctx, w[q + "src_attn.linear_out.weight"], w[q + "src_attn.linear_out.bias"], resid=x, out=x)
            ops.linear(x, w[q + "feed_forward.w_1.weight"], w[q + "feed_forward.w_1.bias"], ln=ln("norm3"), act=self.rescorer.act,
                       out=self.h)
            ops.linear(self.h, w[q + "feed_forward.w_2.weight"], w[q + "feed_forward.w_2.bias"], resid=x, out=x)
        ops.linear(x, w["decoder.output_layer.weight"], w["decoder.output_layer.bias"],
                   ln=(w["decoder.after_norm.weight"], w["decoder.after_norm.bias"], LN_EPS), out=self.logits)
        for call in self._tail:
            call()

    def _reset(self, meta, cap):
        ops.aed_search_reset(self.desc, self.state, meta[0], meta[1], cap)
        for reset, *_ in self._parts:
            reset()
        self.done.zero_()

    def _take_ctc(self, ctc, n_rows, frames, log_probs):
        """Joint decoding: the call's CTC output, (n_rows, V) after flattening, one row per memory row -> self.ctc, its
        log-softmax (m3_log_softmax_bias, once per call; log_probs: the input already holds log-probabilities and is used as it
        is).  The buffers are kept and grown across calls, so that a captured step keeps reading the same addresses.  Refuses a
        missing or unexpected input and a shape that does not fit, before anything is launched."""
        if self.ctc_weight == 0:
            if ctc is not None:
                raise _lib.M3Error("search: CTC output given, but the search was built with ctc_weight = 0")
            return
        if ctc is None:
            raise _lib.M3Error("search: ctc_weight = %g needs the CTC output (ctc_logits / ctc_rows)" % self.ctc_weight)
        V = self.cfg.vocab
        if ctc.shape[-1] != V:
            raise _lib.M3Error("search: the CTC output has %d classes, the attention decoder %d" % (ctc.shape[-1], V))
        if ctc.numel() // V < n_rows:
            raise _lib.M3Error("search: the CTC output has %d frames, the memory %d" % (ctc.numel() // V, n_rows))
        ctc = ctc.to(self.device, torch.float32).reshape(-1, V)[:n_rows]
        if self.jdesc is None or self.jdesc.max_frames < frames:
            self.jdesc = ops.aed_joint_desc(self.desc, self.pre_beam, -(-frames // 64) * 64)
            self.jstate = torch.zeros(ops.aed_joint_state_size(self.jdesc), dtype=torch.uint8, device=self.device)
            self.jscratch = torch.zeros(ops.aed_joint_scratch_size(self.jdesc), dtype=torch.uint8, device=self.device)
            self._graph = None
        if self.ctc is None or self.ctc.shape[0] < n_rows:
            self.ctc = torch.zeros(n_rows, V, dtype=torch.float32, device=self.device)
            self._graph = None
        self.ctc[:n_rows].copy_(ctc.contiguous() if log_probs else ops.log_softmax_bias(ctc.contiguous()))

    def _project(self, rows, raw_memory):
        """The memory's K / V projection for all layers: one GEMM per search, shared by every beam and every step.  The buffer
        is kept (and grown) across calls so that a captured step keeps reading the same addresses."""
        w, L, D = self.rescorer.w, self.cfg.num_blocks, self.cfg.dim
        if self.kvp is None or self.kvp.shape[0] < rows.shape[0]:
            self.kvp = torch.zeros(rows.shape[0], L * 2 * D, dtype=torch.float32, device=self.device)
            self._graph = None
        norm = (w["after_norm.weight"], w["after_norm.bias"], LN_EPS) if raw_memory else None
        # src_kv_all stacks the right-to-left decoder's layers behind the left one's: the search takes the first L only
        ops.linear(rows, w["decoder.src_kv_all.weight"][:L * 2 * D], w["decoder.src_kv_all.bias"][:L * 2 * D], ln=norm,
                   out=self.kvp[:rows.shape[0]])

    def _take_lm_on(self, lm_on):
        """the per-utterance switch of the call -> self.lm_on (kept across calls: a captured step reads the same address)"""
        if self.lm is None:
            if lm_on is not None:
                raise _lib.M3Error("search: lm_on given, but the search was built without an LM")
            return
        if isinstance(self.lm, NgramLmSet):                       # ints: 0 = off, j = member j - 1 (True / 1 = member 0)
            vals = None if lm_on is None else torch.as_tensor(lm_on).reshape(-1).tolist()
            if vals is not None and len(vals) != self.B:
                raise _lib.M3Error("search: lm_on has %d entries for %d utterances" % (len(vals), self.B))
            on = lm_flags(self.lm, vals, self.B, "search", _lib.M3Error)
        else:
            on = [1] * self.B if lm_on is None else [int(bool(v)) for v in torch.as_tensor(lm_on).reshape(-1).tolist()]
        if len(on) != self.B:
            raise _lib.M3Error("search: lm_on has %d entries for %d utterances" % (len(on), self.B))
        self.lm_on.copy_(torch.tensor(on, dtype=torch.int32))

    def _take_graph_ids(self, graph_ids):
        """the per-utterance graph of the call -> self.graph_of (kept across calls: a captured step reads the same address);
        -> the ids as Python ints, -1 for every utterance the kernels treat as unbiased"""
        if self.context is None:
            if graph_ids is not None:
                raise _lib.M3Error("search: graph_ids given, but the search was built without a context")
            return None
        ids = [0] * self.B if graph_ids is None else [int(v) for v in torch.as_tensor(graph_ids).reshape(-1).tolist()]
        if len(ids) != self.B:
            raise _lib.M3Error("search: graph_ids has %d entries for %d utterances" % (len(ids), self.B))
        ids = [min(max(g, -(2 ** 31)), 2 ** 31 - 1) for g in ids]
        self.graph_of.copy_(torch.tensor(ids, dtype=torch.int32))
        return [g if 0 <= g < len(self.context) else -1 for g in ids]

    def _run(self, rows, row0, lens, raw_memory, detail, max_steps, poll, ctc=None, ctc_log_probs=False, lm_on=None, graph_ids=None):
        """rows (n, D) memory rows on the device; row0 / lens: B Python ints each, validated by the caller; ctc: None or the
        CTC output of the same n rows; lm_on: None or B switches; graph_ids: None or B graph ids"""
        cfg, d = self.cfg, self.desc
        cap = self.max_steps if max_steps is None else int(max_steps)
        if not 1 <= cap <= self.max_steps:
            raise _lib.M3Error("search: max_steps = %d outside [1, %d] (the constructor's bound sizes the cache)" % (cap, self.max_steps))
        poll = self.poll if poll is None else max(int(poll), 1)
        self._take_ctc(ctc, rows.shape[0], max(lens), ctc_log_probs)
        self._take_lm_on(lm_on)
        graphs = self._take_graph_ids(graph_ids)
        meta =torch.tensor([row0, lens], dtype=torch.int32).to(self.device)
        self._project(rows, raw_memory)
        self._reset(meta, cap)
        most = min(max(lens), cfg.max_len - 1, cap)
        issued = 0
        while issued < most:
            if self.use_graph:
                self._replay(meta, cap)
            else:
                self._step()
            issued += 1
            if issued % poll == 0 and issued < most and self._all_done():
                break
        self.steps_issued = issued
        res = ops.aed_search_result(d, self.state)
        self.last = dict(res, state=self.state, done=self.done)
        # the float parts behind the score: att, ctc, then what each part alone adds.  The att part comes from the FIRST part
        # present, the one whose state stores it (scorer state, else LM state, else context state); ctc is zeros without CTC
        floats = []
        for _, result, att_key, adds in self._parts:
            gained = result()
            att = gained.pop(att_key)
            self.last.update(gained)
            if not floats:
                self.last.update(att=att, ctc=gained["ctc"] if "ctc" in gained else torch.zeros_like(att))
                floats = ["att", "ctc"]
            floats += adds
        parts = [self.last[k].reshape(-1).view(torch.int32) for k in floats]
        tail = [self.last["ctx_state"].reshape(-1)] if self.context is not None else []   # int32 as it is, behind the float parts
        host = torch.cat([res["hyp_tokens"].reshape(-1), res["hyp_len"].reshape(-1), res["finished"].reshape(-1), res["best"],
                          res["score"].reshape(-1).view(torch.int32)] + parts + tail).cpu()
        B, N, S = self.B, self.beam, self.max_steps
        toks = host[:B * N * S].view(B, N, S)
        o = B * N * S
        hlen, fin, best = host[o:o + B * N].tolist(), host[o + B * N:o + 2 * B * N].tolist(), host[o + 2 * B * N:o + 2 * B * N + B].tolist()
        score = host[o + 2 * B * N + B:].view(torch.float32).tolist()             # score, then (joint) att, ctc, (LM) lm: B * N each
        out = []
        for b in range(B):
            hyps = [(tuple(toks[b, i, :hlen[b * N + i]].tolist()), score[b * N + i], bool(fin[b * N + i])) for i in range(N)]
            if parts:
                hyps = [h + tuple(score[(k + 1) * B * N + b * N + i] for k in range(len(parts))) for i, h in enumerate(hyps)]
            if tail:                                                # final = bonus - pot[ctx_state]: what is no longer provisional
                pot = self.context.graphs[graphs[b]].pot if graphs[b] >= 0 else None
                states = host[-B * N:].tolist()
                hyps = [h + (h[-1] - float(pot[states[b * N + i]]) if pot is not None and 0 <= states[b * N + i] < len(pot) else h[-1],)
                        for i, h in enumerate(hyps)]
            out.append((list(hyps[best[b]][0]), hyps) if detail else list(hyps[best[b]][0]))
        return out

    def _all_done(self):
        self._done_host.copy_(self.done, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return bool(self._done_host.all())

    def _replay(self, meta, cap):
        """use_graph: the step as one captured graph.  The first graph call of an object warms the launchers up with one eager
        step (kernel attributes are set once per device, outside any capture), restores the start and captures."""
        if self._graph is None:
            self._step()
            self._reset(meta, cap)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step()
            self._graph = g
        self._graph.replay()

    # ---- the public calls
    def search(self, memory, mem_len, raw_memory=False, detail=False, max_steps=None, poll=None, ctc_logits=None,
               ctc_log_probs=False, lm_on=None, graph_ids=None):
        """memory (B, T', D) on the device: the encoder's normalised hidden states (Engine.hidden()), or with raw_memory the
        residual stream before after_norm (Engine.hidden(normalized=False)), the LayerNorm then riding in the K / V GEMM's
        prologue; mem_len (B,) valid frames.  Utterance b stops once its `beam` hypotheses have all ended in eos, or after
        min(mem_len[b], max_len - 1, max_steps) steps with whatever it has; max_steps: a bound for this call, at most the
        constructor's.
        -> the best token list per utterance; detail: (best tokens, [(tokens, score, finished)] in slot order) per utterance.
        Joint decoding (ctc_weight > 0): ctc_logits (B, T', V), the CTC output over the memory's frames (another frame count or
        vocabulary is refused); ctc_log_probs: it already holds log-probabilities and is used as it is.  The score is then the
        joint key and detail gives (tokens, key, finished, att, ctc).
        LM fusion (lm given): lm_on, None or B flags, 0 = this utterance is searched without the LM; detail appends lm, the LM's
        log-probability of the hypothesis: (tokens, key, finished, att, ctc, lm), ctc = 0.0 when ctc_weight = 0.
        Hotword biasing (context given): graph_ids, None (graph 0 for all) or B graph ids, -1 (or any id outside the set) = this
        utterance is searched unbiased; detail appends the context part after the parts above: bonus, what the key holds, and
        final = bonus - pot[ctx_state], what is no longer provisional (equal for a finished hypothesis):
        (tokens, key, finished, att, ctc[, lm], bonus, final).
        mem_len < 1 is refused before anything is launched.  The device tensors of the call stay in self.last."""
        cfg, B = self.cfg, self.B
        memory = memory.to(self.device, torch.float32)
        if memory.dim() != 3 or memory.shape[0] != B or memory.shape[2] != cfg.dim:
            raise ValueError("search: memory %s for %d utterances of dim %d" % (tuple(memory.shape), B, cfg.dim))
        Tm = int(memory.shape[1])
        lens = [int(v) for v in torch.as_tensor(mem_len).reshape(-1).tolist()]
        if len(lens) != B:
            raise ValueError("search: %d memory lengths for %d utterances" % (len(lens), B))
        for b, m in enumerate(lens):
            if not 1 <= m <= Tm:
                raise _lib.M3Error("search: utterance %d has %d memory frames (mem_len = 0 is rejected; the memory holds %d)" % (b, m, Tm))
        if ctc_logits is not None and self.ctc_weight > 0 and (ctc_logits.dim() != 3 or ctc_logits.shape[0] != B or ctc_logits.shape[1] != Tm):
            raise _lib.M3Error("search: the CTC output %s does not cover the memory's %d x %d frames" % (tuple(ctc_logits.shape), B, Tm))
        return self._run(memory.contiguous().view(B * Tm, cfg.dim), [b * Tm for b in range(B)], lens, raw_memory, detail, max_steps, poll,
                         ctc_logits, ctc_log_probs, lm_on, graph_ids)

    def search_rows(self, rows, row0, raw_memory=True, detail=False, max_steps=None, poll=None, ctc_rows=None, ctc_log_probs=False,
                    lm_on=None, graph_ids=None):
        """The search over PACKED memory rows, as AttentionRescorer.rescore_rows takes them: rows (>= R, D) on the device,
        row0 (B + 1,) int32 (m3_aed_memory_gather leaves them so): utterance b owns rows [row0[b], row0[b + 1]).  raw_memory:
        the rows are the residual stream before after_norm (what the streaming store keeps).  An utterance without a row is
        refused before anything is launched.  Joint decoding: ctc_rows (>= row0[B], V), the CTC output of the same packed rows.
        lm_on and graph_ids: as search takes them."""
        cfg, B = self.cfg, self.B
        if rows.dim() != 2 or rows.shape[1] != cfg.dim or not rows.is_contiguous() or row0.numel() != B + 1:
            raise ValueError("search_rows: rows %s / row0 (%d,) for %d utterances of dim %d" % (tuple(rows.shape), row0.numel(), B, cfg.dim))
        r0 = [int(v) for v in row0.reshape(-1).tolist()]
        if r0[0] != 0 or any(a > b for a, b in zip(r0, r0[1:])) or r0[-1] > rows.shape[0]:
            raise _lib.M3Error("search_rows: row0 = %s does not describe %d packed rows" % (r0, rows.shape[0]))
        lens = [b - a for a, b in zip(r0, r0[1:])]
        for b, m in enumerate(lens):
            if m < 1:
                raise _lib.M3Error("search_rows: utterance %d has no memory row (mem_len = 0 is rejected)" % b)
        if ctc_rows is not None and self.ctc_weight > 0 and ctc_rows.dim() != 2:
            raise _lib.M3Error("search_rows: the CTC output %s is not (rows, vocab)" % (tuple(ctc_rows.shape),))
        return self._run(rows[:r0[-1]].to(self.device, torch.float32), r0[:-1], lens, raw_memory, detail, max_steps, poll,
                         ctc_rows, ctc_log_probs, lm_on, graph_ids)
