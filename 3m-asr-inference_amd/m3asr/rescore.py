"""Attention rescoring on the device: the AED decoder's teacher-forced pass over the CTC n-best (the reference's decoding
mode `attention_rescoring`, trainer_3m_fix/model/ctc_aed.py:160-252, with the decoder of layer/att_decoder.py).

The reference repeats the encoder output `beam` times and pads every hypothesis to the longest.  Here the decoder runs on
PACKED hypothesis rows (len + 1 rows per live hypothesis, none for an empty n-best slot), the memory of an utterance is
projected to K / V once per call for all layers (one GEMM) and shared by its whole beam, and the (rows, V) log-probabilities
never leave the device: m3_aed_score reduces them to one score per hypothesis and one choice per utterance.

    cfg, packed, extra = load_plan(path)
    rescorer = AttentionRescorer(packed, decoder_config_of(extra), device)
    results = rescorer.rescore(engine.hidden(), out_lens, search, ctc_weight=0.5)

Dense layers are m3_linear calls (LayerNorm prologue, bias, ReLU / SiLU, residual); the rest is csrc/aed_rescore.hip.  The
decoder computes in fp32 whatever the plan's weight_dtype.  There is no torch fallback."""
import torch

from . import _lib, ops
from .config import DecoderConfig

LN_EPS = 1e-12


class AttentionRescorer:
    def __init__(self, packed, dcfg: DecoderConfig, device="cuda:0"):
        """packed: a plan's tensors holding plan.pack_decoder's entries (`decoder.*`, `after_norm.*`); dcfg: its DecoderConfig
        (plan.decoder_config_of(extra)).  A plan built from an encoder-only checkpoint has neither: M3Error."""
        if dcfg is None or "decoder.embed.weight" not in packed:
            raise _lib.M3Error("AttentionRescorer: the plan has no attention decoder (no extra['decoder'] / decoder.* tensors); "
                               "build it from a CTC/attention checkpoint (builder.py packs the decoder when the checkpoint has one)")
        self.cfg = dcfg
        self.device = torch.device(device)
        D, F, dk = dcfg.dim, dcfg.linear_units, dcfg.d_k
        if dk % 16 or dk > 128:
            raise _lib.M3Error("AttentionRescorer: head size %d; the attention kernel takes multiples of 16 up to 128" % dk)
        if D % 16 or F % 16 or D > 1024:
            raise _lib.M3Error("AttentionRescorer: dim %d / linear_units %d; the GEMMs take multiples of 16, dim <= 1024" % (D, F))
        if dcfg.r_num_blocks > 0 and "decoder.right.embed.weight" not in packed:
            raise _lib.M3Error("AttentionRescorer: the config has %d right-to-left blocks, the plan none" % dcfg.r_num_blocks)
        self.w = {k: v.to(self.device, torch.float32).contiguous() for k, v in packed.items()
                  if k.startswith("decoder.") or k.startswith("after_norm.")}
        self.act = {"relu": _lib.ACT_RELU, "silu": _lib.ACT_SILU}[dcfg.activation]
        self.last = None      # device tensors of the last call: dict(att, r_att, final (B,beam), best (B,), prior (B,beam))

    # ---- the n-best and its packed layout
    @staticmethod
    def _nbest(source):
        """(hyp_tokens, hyp_len, prior, n_hyps) on the device from a CtcBeamSearch (prior = its ranking key) or from the
        tensors (hyp_tokens, hyp_len, hyp_score, n_hyps) (prior = hyp_score)."""
        if hasattr(source, "nbest_tensors"):
            t = source.nbest_tensors(detail=True)
            toks, hlen, score, bonus, n = t[0], t[1], t[2], t[3], t[-1]
            prior = score + bonus
            if len(t) == 6:       # fused search: + lm_weight * log P_LM + length_bonus * |y|
                w = source.lm_weights() if hasattr(source, "lm_weights") else source.lm_weight   # an LM set: one weight per utterance
                prior = prior + (w * t[4] + source.length_bonus * hlen.to(torch.float32))
            return toks, hlen, prior.contiguous(), n
        toks, hlen, score, n = source
        return toks, hlen, score, n

    def _layout(self, hl, nh, kv):
        """Host side of the packed rows: hl hyp_len (B x beam lists), nh n_hyps (B), kv (first memory row, memory frames) of
        every utterance -- all read from the device by the caller in ONE device-to-host copy."""
        B, beam = len(hl), (len(hl[0]) if hl else 0)
        row0, self_d, src_d = [0], [], []
        for b in range(B):
            live = max(min(nh[b], beam), 0)
            for i in range(beam):
                nq = hl[b][i] + 1 if i < live else 0
                if nq > self.cfg.max_len:
                    raise _lib.M3Error("rescore: a hypothesis of %d tokens exceeds the positional table (%d)" % (nq - 1, self.cfg.max_len))
                r = row0[-1]
                self_d.append((r, nq, r, nq, 1))
                src_d.append((r, nq, kv[b][0], kv[b][1] if nq else 0, 0))
                row0.append(r + nq)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(self.device)   # noqa: E731
        max_q = max((d[1] for d in self_d), default=0)
        return row0[-1], max_q, i32(row0), i32(self_d).view(-1, 5), i32(src_d).view(-1, 5)

    def _read(self, hlen, n_hyps, extra):
        """(hyp_len lists, n_hyps list, extra list) from one device-to-host copy of the three int32 tensors"""
        B, beam = hlen.shape
        parts = [hlen.reshape(-1), n_hyps.reshape(-1)] + ([extra.reshape(-1).to(torch.int32)] if extra.is_cuda else [])
        flat = torch.cat(parts).cpu().tolist()
        hl = [flat[b * beam:(b + 1) * beam] for b in range(B)]
        return hl, flat[B * beam:B * beam + B], (flat[B * beam + B:] if extra.is_cuda else extra.reshape(-1).tolist())

    # ---- one decoder over the packed rows
    def _decode(self, p, blocks, kv, kv_layer0, toks, hlen, n_hyps, row0, rows, max_q, self_d, src_d, reverse):
        w, D, H = self.w, self.cfg.dim, self.cfg.heads
        x, target = ops.aed_embed(toks, hlen, n_hyps, row0, w[p + "embed.weight"], w["decoder.pe"], rows, reverse)
        for i in range(blocks):
            q = p + "layers.%d." % i
            ln = lambda n: (w[q + n + ".weight"], w[q + n + ".bias"], LN_EPS)   # noqa: E731
            qkv = ops.linear(x, w[q + "self_attn.qkv.weight"], w[q + "self_attn.qkv.bias"], ln=ln("norm1"))
            ctx = ops.aed_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self_d, max_q, H)
            ops.linear(ctx, w[q + "self_attn.linear_out.weight"], w[q + "self_attn.linear_out.bias"], resid=x, out=x)
            qs = ops.linear(x, w[q + "src_attn.linear_q.weight"], w[q + "src_attn.linear_q.bias"], ln=ln("norm2"))
            c0 = (kv_layer0 + i) * 2 * D
            ctx = ops.aed_attention(qs, kv[:, c0:c0 + D], kv[:, c0 + D:c0 + 2 * D], src_d, max_q, H)
            ops.linear(ctx, w[q + "src_attn.linear_out.weight"], w[q + "src_attn.linear_out.bias"], resid=x, out=x)
            h = ops.linear(x, w[q + "feed_forward.w_1.weight"], w[q + "feed_forward.w_1.bias"], ln=ln("norm3"), act=self.act)
            ops.linear(h, w[q + "feed_forward.w_2.weight"], w[q + "feed_forward.w_2.bias"], resid=x, out=x)
        logits = ops.linear(x, w[p + "output_layer.weight"], w[p + "output_layer.bias"],
                            ln=(w[p + "after_norm.weight"], w[p + "after_norm.bias"], LN_EPS))
        return logits, target

    def _score(self, rows_kv, raw_memory, toks, hlen, prior, n_hyps, hl, nh, kv, ctc_weight, reverse_weight):
        """The decoder pass and the choice over memory rows (R, D): the K / V GEMM runs over exactly these rows."""
        cfg, w = self.cfg, self.w
        B, beam = hlen.shape
        rows, max_q, row0, self_d, src_d = self._layout(hl, nh, kv)
        logits = target = r_logits = r_target = None
        if rows > 0:
            norm = (w["after_norm.weight"], w["after_norm.bias"], LN_EPS) if raw_memory else None
            kvp = ops.linear(rows_kv, w["decoder.src_kv_all.weight"], w["decoder.src_kv_all.bias"], ln=norm)
            args = (toks, hlen, n_hyps, row0, rows, max_q, self_d, src_d)
            logits, target = self._decode("decoder.", cfg.num_blocks, kvp, 0, *args, reverse=False)
            if reverse_weight > 0:
                r_logits, r_target = self._decode("decoder.right.", cfg.r_num_blocks, kvp, cfg.num_blocks, *args, reverse=True)
        else:
            logits = torch.empty(0, cfg.vocab, dtype=torch.float32, device=self.device)
        att, r_att, final, best = ops.aed_score(logits, target, row0, n_hyps, B, beam, prior=prior, ctc_weight=ctc_weight,
                                                r_logits=r_logits, r_target=r_target, reverse_weight=reverse_weight)
        self.last = dict(att=att, r_att=r_att, final=final, best=best, prior=prior)
        toks_h, prior_h, att_h, final_h, best_h = toks.cpu(), prior.cpu(), att.cpu(), final.cpu(), best.cpu().tolist()
        out = []
        for b in range(B):
            hyps = [(tuple(toks_h[b, i, :hl[b][i]].tolist()), float(prior_h[b, i]), float(att_h[b, i]), float(final_h[b, i]))
                    for i in range(max(min(nh[b], beam), 0))]
            out.append((hyps[best_h[b]][0] if best_h[b] >= 0 else (), hyps))
        return out

    def _check_weights(self, reverse_weight):
        if reverse_weight > 0 and self.cfg.r_num_blocks == 0:
            raise _lib.M3Error("rescore: reverse_weight = %g needs a right-to-left decoder (r_num_blocks = 0)" % reverse_weight)

    def rescore(self, memory, mem_len, nbest, ctc_weight=0.0, reverse_weight=0.0, raw_memory=False):
        """memory (B, T', D) on the device: the encoder's normalised hidden states (Engine.hidden()), or with raw_memory the
        residual stream before after_norm (Engine.hidden(normalized=False)) -- the LayerNorm then rides in the K / V GEMM's
        prologue; mem_len (B,) valid frames; nbest: a CtcBeamSearch, or its tensors (hyp_tokens, hyp_len, hyp_score, n_hyps).
        final = (1 - reverse_weight) att + reverse_weight r_att + ctc_weight prior.
        -> per utterance (best tokens, [(tokens, prior, att, final)] in n-best order); an utterance without hypotheses gives
        ((), []).  The device tensors of the call stay in self.last."""
        cfg = self.cfg
        self._check_weights(reverse_weight)
        toks, hlen, prior, n_hyps = self._nbest(nbest)
        B, beam, _ = toks.shape
        memory = memory.to(self.device, torch.float32)
        if memory.dim() != 3 or memory.shape[0] != B or memory.shape[2] != cfg.dim:
            raise ValueError("rescore: memory %s for %d utterances of dim %d" % (tuple(memory.shape), B, cfg.dim))
        Tm = int(memory.shape[1])
        mem_len = torch.as_tensor(mem_len).reshape(-1)
        if mem_len.numel() != B:
            raise ValueError("rescore: %d memory lengths for %d utterances" % (mem_len.numel(), B))
        hl, nh, ml = self._read(hlen, n_hyps, mem_len)
        for b in range(B):
            if min(nh[b], beam) > 0 and not 1 <= ml[b] <= Tm:
                # a query row with no visible key has no softmax: refuse before anything is launched
                raise _lib.M3Error("rescore: utterance %d has %d memory frames (kv_len = 0 is rejected; the memory holds %d)"
                                   % (b, ml[b], Tm))
        return self._score(memory.contiguous().view(B * Tm, cfg.dim), raw_memory, toks, hlen, prior, n_hyps, hl, nh,
                           [(b * Tm, ml[b]) for b in range(B)], ctc_weight, reverse_weight)

    def rescore_rows(self, rows, row0, nbest, streams=None, ctc_weight=0.0, reverse_weight=0.0, raw_memory=True):
        """Rescore the listed streams of a search over PACKED memory rows (streaming two-pass decoding).
        rows (>= R, D) on the device, row0 (n + 1,) int32 on the device as m3_aed_memory_gather leaves them: listed stream j
        owns rows [row0[j], row0[j + 1]), R = row0[n]; raw_memory: the rows are the residual stream before after_norm (what
        the store keeps).  streams: the n streams of `nbest` the rows belong to, in that order (default: all of them).  The
        K / V GEMM runs over the R rows only.  A listed stream with hypotheses but no memory row (it was closed before its
        first chunk, or its store overflowed) is not an error: its result is ((), []), as for a stream without hypotheses.
        -> per LISTED stream what rescore() returns per utterance; self.last holds the listed streams' tensors."""
        cfg = self.cfg
        self._check_weights(reverse_weight)
        toks, hlen, prior, n_hyps = self._nbest(nbest)
        if streams is not None:
            streams = [int(b) for b in streams]
            if any(not 0 <= b < toks.shape[0] for b in streams):
                raise ValueError("rescore_rows: streams %s outside [0, %d)" % (streams, toks.shape[0]))
            sel = torch.tensor(streams, dtype=torch.int64).to(self.device)
            toks, hlen, prior, n_hyps = (t.index_select(0, sel).contiguous() for t in (toks, hlen, prior, n_hyps))
        n, beam, _ = toks.shape
        if rows.dim() != 2 or rows.shape[1] != cfg.dim or not rows.is_contiguous() or row0.numel() != n + 1:
            raise ValueError("rescore_rows: rows %s / row0 (%d,) for %d streams of dim %d" % (tuple(rows.shape), row0.numel(), n, cfg.dim))
        hl, nh, r0 = self._read(hlen, n_hyps, row0)
        if r0[0] != 0 or any(a > b for a, b in zip(r0, r0[1:])) or r0[-1] > rows.shape[0]:
            raise _lib.M3Error("rescore_rows: row0 = %s does not describe %d packed rows" % (r0, rows.shape[0]))
        kv = [(r0[j], r0[j + 1] - r0[j]) for j in range(n)]
        dead = [j for j in range(n) if nh[j] > 0 and kv[j][1] == 0]
        if dead:                      # hypotheses without memory: the stream counts as one without hypotheses
            for j in dead:
                nh[j] = 0
            n_hyps = torch.tensor(nh, dtype=torch.int32).to(self.device)
        return self._score(rows[:r0[-1]], raw_memory, toks, hlen, prior, n_hyps, hl, nh, kv, ctc_weight, reverse_weight)
