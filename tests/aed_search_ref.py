"""Restatement of the attention-decoding contract in plain torch, float64-capable (the checker of m3asr.aed_search; nothing
here is used by the product).  Built on aed_ref.decoder_logp; written from the reference's text, trainer_3m_fix:

  layer/att_decoder.py:258-299   forward_one_step: the decoder on the prefix, log_softmax of the LAST row; its cache
                                 (:95-107,139-140) holds the layers' outputs of the earlier positions and follows the hypothesis,
                                 so it computes what the decoder computes on the whole prefix.  This restatement recomputes the
                                 prefix at every step -- that is the point of it: no cache, no ancestry, nothing to get wrong.
  layer/att_decoder.py:389-411   a bidirectional decoder searches with its left decoder only
  utils/mask.py:205-251          mask_finished_scores / mask_finished_preds: a finished hypothesis offers exactly one candidate,
                                 increment 0, token eos

One utterance, m memory frames, beam N, sos = eos = V - 1:
  start   slot 0 = [sos] with score 0, slots 1 .. N-1 = [sos] with score -inf, nobody finished
  step    per slot logp = decoder_logp([sos, y..], memory)[-1]; its N largest with their tokens, largest first, ties to the lower
          token id; a finished slot offers (0, eos) alone; candidate = slot score + increment; keep the N largest of the N * N,
          largest first, ties to the lower flat index slot * N + rank; new slot j = j-th kept candidate: the parent's tokens
          plus the new one, finished if that is eos
  stop    after the step at which all N slots are finished, or after step limit = min(m, max_len - 1, max_steps)
  result  the N slots in slot order: (tokens without sos and without trailing eos, score, finished); best = the first slot with
          the strictly largest score; at the limit unfinished hypotheses are returned as they are
The right-to-left decoder and ctc_weight take no part.

FROZEN UTTERANCES.  An utterance that has stopped is frozen: a further step of a batch it sits in does not change it.  So a
batch stepped in lock step for max(limit) steps (or more) gives every utterance exactly what it gets alone; search() below
IS that lock-step loop (frozen_step), and tests/test_aed_search_host.py checks it against every utterance searched alone and
against extra steps.

DECISION MARGIN.  At each step pool the candidates of all live slots (score > -inf): every token of an unfinished slot, the
single eos candidate of a finished one.  Sort the pooled scores; the smallest gap between consecutive entries among the top
N + 1 is the step's margin, the utterance's margin is the minimum over its steps.  The two-stage top-k above selects exactly
the global top N of that pool in that order, so two implementations whose scores differ by less than half the margin cannot
differ in any discrete choice."""
import torch

import aed_ref

INF = float("inf")


def _largest(values, k):
    """indices of the k largest entries, largest first, ties to the lower index"""
    return torch.sort(values, descending=True, stable=True)[1][:k].tolist()


def start(beam, limit, dtype):
    score = torch.full((beam,), -INF, dtype=dtype)
    score[0] = 0
    return dict(tokens=[[] for _ in range(beam)], score=score, finished=[False] * beam, steps=0, limit=limit, done=limit < 1,
                margin=INF, history=[])


def advance(state, logp_of, beam, eos):
    """One step of one live utterance -> the new state (the old one is not touched).  logp_of(tokens) -> (V,) log-probabilities
    of the next token after [sos] + tokens."""
    N, score = beam, state["score"]
    cand_score = torch.full((N * N,), -INF, dtype=score.dtype)
    cand_tok = [eos] * (N * N)
    pool = []
    for i in range(N):
        if state["finished"][i]:
            cand_score[i * N] = score[i]
            pool.append(score[i:i + 1])
        elif score[i] > -INF:
            logp = logp_of(state["tokens"][i]).to(score.device)
            top = _largest(logp, N)
            cand_score[i * N:i * N + len(top)] = score[i] + logp[top]
            cand_tok[i * N:i * N + len(top)] = top
            pool.append(score[i] + logp)
        # a slot at -inf offers -inf candidates only: with N <= V there are always N finite ones ahead of them
    pool = torch.sort(torch.cat(pool), descending=True)[0][:N + 1]
    margin = state["margin"]
    if pool.numel() > 1:
        margin = min(margin, float((pool[:-1] - pool[1:]).min()))
    kept = _largest(cand_score, N)
    assert bool(torch.isfinite(cand_score[kept]).all()), "fewer than N finite candidates"
    tokens = [state["tokens"][c // N] + [cand_tok[c]] for c in kept]
    finished = [cand_tok[c] == eos for c in kept]
    steps = state["steps"] + 1
    entry = dict(tokens=[list(t) for t in tokens], score=cand_score[kept].clone(), finished=list(finished), parent=[c // N for c in kept])
    return dict(tokens=tokens, score=cand_score[kept].clone(), finished=finished, steps=steps, limit=state["limit"],
                done=all(finished) or steps >= state["limit"], margin=margin, history=state["history"] + [entry])


def frozen_step(state, logp_of, beam, eos):
    """the step of an utterance inside a batch: a stopped utterance is left alone"""
    return state if state["done"] else advance(state, logp_of, beam, eos)


def strip(tokens, eos):
    n = len(tokens)
    while n > 0 and tokens[n - 1] == eos:
        n -= 1
    return tuple(tokens[:n])


def result(state, eos):
    score = state["score"].tolist()
    best = 0
    for i, s in enumerate(score):
        if s > score[best]:
            best = i
    nbest = [(strip(t, eos), s, f) for t, s, f in zip(state["tokens"], score, state["finished"])]
    return dict(nbest=nbest, best=best, margin=state["margin"], steps=state["steps"], limit=state["limit"], history=state["history"])


def _left(dcfg, prefix):
    return prefix + ("left_decoder." if dcfg.r_num_blocks > 0 else "")


def limit_of(dcfg, m, max_steps=None):
    return min(int(m), dcfg.max_len - 1, int(max_steps) if max_steps is not None else int(m))


def search(sd, dcfg, memory, mem_len, beam, max_steps=None, dtype=torch.float64, prefix="decoder.", extra_steps=0):
    """memory (B, T, D) normalised encoder states, mem_len (B,) -> per utterance dict(nbest=[(tokens, score, finished)], best,
    margin, steps, limit, history=[per step dict(tokens (with trailing eos), score, finished, parent)]).  The batch moves in
    lock step for max(limit) + extra_steps steps; see FROZEN UTTERANCES."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    eos, left = dcfg.vocab - 1, _left(dcfg, prefix)
    assert 1 <= beam <= dcfg.vocab
    mems = [memory[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]

    def logp_of(b):
        return lambda y: aed_ref.decoder_logp(sd, left, dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + list(y), mems[b])[-1]

    states = [start(beam, limit_of(dcfg, mem_len[b], max_steps), dtype) for b in range(len(mems))]
    for _ in range(max(s["limit"] for s in states) + extra_steps):
        states = [frozen_step(s, logp_of(b), beam, eos) for b, s in enumerate(states)]
    return [result(s, eos) for s in states]


def teacher_forced_scores(sd, dcfg, memory, mem_len, results, dtype=torch.float32, prefix="decoder."):
    """The scores of the kept candidates of every step of `results` (search()'s, usually float64), recomputed teacher-forced
    in `dtype`: per utterance, per step, a list of N floats.  A hypothesis's score is the sum, left to right, of logp[j][y_j] up to
    and including its first eos: the increments the search itself added.  The yardstick's e32 is the largest difference between
    these in float32 and the float64 search's own."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    eos, left = dcfg.vocab - 1, _left(dcfg, prefix)
    out = []
    for b, res in enumerate(results):
        mem = memory[b, :int(mem_len[b])].to(dtype)
        memo = {}
        per_step = []
        for entry in res["history"]:
            scores = []
            for toks in entry["tokens"]:
                y = list(toks)
                if eos in y:
                    y = y[:y.index(eos) + 1]
                key = tuple(y)
                if key not in memo:
                    logp = aed_ref.decoder_logp(sd, left, dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + y[:-1], mem)
                    s = logp.new_zeros(())
                    for j, t in enumerate(y):
                        s = s + logp[j][t]
                    memo[key] = float(s)
                scores.append(memo[key])
            per_step.append(scores)
        out.append(per_step)
    return out


def e32_of(results64, scores32):
    """largest |float64 score - float32 teacher-forced score| over every kept candidate of every step of every utterance"""
    e = 0.0
    for res, per_step in zip(results64, scores32):
        for entry, s32 in zip(res["history"], per_step):
            e = max(e, max(abs(float(a) - b) for a, b in zip(entry["score"], s32)))
    return e
