"""Restatement of attention decoding with n-gram LM fusion and a length bonus, float64-capable (the checker of m3asr.aed_search
with lm=; nothing here is used by the product).  THE CONTRACT is everything of tests/aed_joint_ref.py (start, limits, stop rule,
max_steps, frozen utterances, stripping, pick order, tie-breaks: DESIGN.md 21 and 23), plus the following.

HYPOTHESIS STATE.  Besides its tokens, key, att, ctc and CTC scorer state a hypothesis carries
    lm_state   int, a state of the LM automaton (m3asr.lm); the image's `start` for [sos]
    lm         double, the LM's log-probability of its tokens; 0.0 for [sos]
    n          int, its tokens after sos, eos included; 0 for [sos]

EXTENDING A LIVE SLOT by candidate c, one of the slot's P largest attention log-probabilities (exactly the joint search's picks):
    n' = n + 1
    c != eos:  (d, lm_state') = lm_step(lm_state, c),  lm' = lm + d.  lm_step is the score contract of the CTC search's fusion
               (m3asr/lm.py, csrc/kernels.h), unchanged and for every token id, 0 included: from lm_state down its back-off chain,
               the back-off weights summed in double in walk order, then the found arc's value added; at state 0 the dense
               unigram, or unk_logp for a token outside [0, V).  The sum lm + d is in double.
    c == eos:  lm' = lm + (double)final[lm_state] * use_eos,  lm_state' = lm_state.

KEY.  key' = jkey + (float)(alpha * lm' + beta * n'),  jkey the joint search's (1 - w) att' + w ctc' (-inf when a part is).
alpha and beta are doubles; the expression in the parentheses is evaluated in double as written, two products and one sum, no
fused multiply-add, and rounded to float32 ONCE; a -inf jkey gives a -inf key.  (In this restatement jkey is in the search's
dtype; the rounded LM term is added to it in that dtype.)

FINISHED SLOTS offer (0, eos) alone and keep key, lm, lm_state and n as they are.

PER-UTTERANCE SWITCH.  An utterance with lm_on = 0 adds nothing: lm stays 0.0, lm_state stays `start`, key = jkey, and its tokens,
keys, att and ctc are the joint search's, bit for bit (n still counts the tokens).

ctc_weight = 0 WITH AN LM is legal: attention plus LM.  No CTC input, no rn / rb recursion; the ctc part is 0 and jkey = att'.
The row still offers P candidates: the LM is a partial scorer over the pre-beam.

DECISION MARGIN: the joint search's, over the new keys; the pre-beam gap is kept."""
import numpy as np
import torch

import aed_joint_ref
import aed_ref
import aed_search_ref

INF = float("inf")


def lm_term(alpha, beta, lm, n):
    """(float)(alpha * lm + beta * n) as a Python float: Python's doubles do not contract"""
    a = float(alpha) * float(lm)
    b = float(beta) * float(n)
    return float(np.float32(a + b))


def lm_extend(lm, state, total, c, eos, use_eos):
    """-> (lm_state', lm', back-off levels taken, landed on unk_logp)"""
    if c == eos:
        return state, total + float(lm.final[state]) * (1 if use_eos else 0), 0, False
    d, nxt, levels = lm.step(state, int(c))
    unk = _root_reached(lm, state, int(c)) and float(lm.uni_logp[c]) == lm.unk_logp      # no unigram: the table holds unk_logp there
    return nxt, total + d, levels, unk


def _root_reached(lm, state, tok):
    st = int(state)
    while st != 0:
        lo, hi = int(lm.arc_begin[st]), int(lm.arc_begin[st + 1])
        if tok in lm.arc_tok[lo:hi].tolist():
            return False
        st = int(lm.bo_state[st])
    return True


def start(x, beam, limit, lm, dtype):
    att = torch.full((beam,), -INF, dtype=dtype)
    att[0] = 0
    return dict(tokens=[[] for _ in range(beam)], key=att.clone(), att=att, ctc=torch.zeros(beam, dtype=dtype), finished=[False] * beam,
                states=[aed_joint_ref.initial_state(x) if x is not None else None for _ in range(beam)],
                lm_state=[lm.start] * beam, lm=[0.0] * beam, n=[0] * beam, steps=0, limit=limit, done=limit < 1, margin=INF, history=[])


def advance(state, x, logp_of, beam, pre_beam, w, lm, alpha, beta, use_eos, lm_on, eos):
    """One step of one live utterance -> the new state (the old one is not touched).  x: the utterance's CTC log-probabilities,
    None exactly when w == 0."""
    N, P = beam, pre_beam
    dtype = state["att"].dtype
    cands = []          # (flat, key, att, ctc, token, parent, scorer state, lm_state, lm, n, levels, unk)
    margin = state["margin"]
    for i in range(N):
        if state["finished"][i]:
            cands.append((i * P, state["key"][i].clone(), state["att"][i].clone(), state["ctc"][i].clone(), eos, i, None,
                          state["lm_state"][i], state["lm"][i], state["n"][i], 0, False))
            continue
        logp = logp_of(state["tokens"][i]).to(dtype)
        order = torch.sort(logp, descending=True, stable=True)[1].tolist()
        top = order[:P]
        if P < len(order):
            margin = min(margin, float(logp[order[P - 1]] - logp[order[P]]))
        if w > 0:
            psi, states = aed_joint_ref.extend(x, state["states"][i], top)
        else:
            psi, states = torch.zeros(len(top), dtype=dtype), [None] * len(top)
        for k, c in enumerate(top):
            att = state["att"][i] + logp[c]
            jkey = aed_joint_ref.key_of(att, psi[k], w) if w > 0 else att.clone()
            n2 = state["n"][i] + 1
            st2, lm2, levels, unk = state["lm_state"][i], state["lm"][i], 0, False
            key = jkey
            if lm_on:
                st2, lm2, levels, unk = lm_extend(lm, state["lm_state"][i], state["lm"][i], c, eos, use_eos)
                if float(jkey) != -INF:
                    key = jkey + torch.tensor(lm_term(alpha, beta, lm2, n2), dtype=dtype)
            cands.append((i * P + k, key, att, psi[k].clone(), c, i, states[k], st2, lm2, n2, levels, unk))
    keys = torch.stack([c[1] for c in cands])
    assert not bool(torch.isnan(keys).any())
    order = torch.sort(keys, descending=True, stable=True)[1].tolist()      # cands are in flat-index order: stable = lower index
    pool = keys[order[:N + 1]]
    for a, b in zip(pool[:-1].tolist(), pool[1:].tolist()):
        if not (a == -INF and b == -INF):
            margin = min(margin, a - b)
    kept = [cands[j] for j in order[:N]]
    assert len(kept) == N
    tokens = [state["tokens"][c[5]] + [c[4]] for c in kept]
    finished = [c[4] == eos for c in kept]
    new = dict(tokens=tokens, key=torch.stack([c[1] for c in kept]), att=torch.stack([c[2] for c in kept]),
               ctc=torch.stack([c[3] for c in kept]), finished=finished, states=[c[6] for c in kept],
               lm_state=[c[7] for c in kept], lm=[c[8] for c in kept], n=[c[9] for c in kept], steps=state["steps"] + 1,
               limit=state["limit"])
    entry = dict(tokens=[list(t) for t in tokens], key=new["key"].clone(), att=new["att"].clone(), ctc=new["ctc"].clone(),
                 finished=list(finished), parent=[c[5] for c in kept], flat=[c[0] for c in kept], lm_state=list(new["lm_state"]),
                 lm=list(new["lm"]), n=list(new["n"]), levels=[c[10] for c in kept], unk=[c[11] for c in kept])
    new.update(done=all(finished) or new["steps"] >= new["limit"], margin=margin, history=state["history"] + [entry])
    return new


def result(state, eos):
    key = state["key"].tolist()
    best = 0
    for i, s in enumerate(key):
        if s > key[best]:
            best = i
    nbest = [(aed_search_ref.strip(t, eos), k, a, c, f, l)
             for t, k, a, c, f, l in zip(state["tokens"], key, state["att"].tolist(), state["ctc"].tolist(), state["finished"], state["lm"])]
    return dict(nbest=nbest, best=best, margin=state["margin"], steps=state["steps"], limit=state["limit"], history=state["history"],
                states=state["states"], tokens=state["tokens"], lm_state=state["lm_state"], n=state["n"])


def search_with(xs, logp_ofs, limits, beam, pre_beam, w, lm, alpha, beta, eos, use_eos=True, lm_on=None, extra_steps=0,
                dtype=torch.float64):
    """the lock-step loop over utterances given as (x or None, logp_of, limit) triples; a stopped utterance is left alone"""
    on = [1] * len(limits) if lm_on is None else [int(bool(v)) for v in lm_on]
    assert len(on) == len(limits) and all((x is None) == (w == 0) for x in xs)
    states = [start(x, beam, lim, lm, dtype) for x, lim in zip(xs, limits)]
    for _ in range(max(limits) + extra_steps):
        states = [s if s["done"] else advance(s, x, f, beam, pre_beam, w, lm, alpha, beta, use_eos, o, eos)
                  for s, x, f, o in zip(states, xs, logp_ofs, on)]
    return [result(s, eos) for s in states]


def search(sd, dcfg, memory, mem_len, ctc_logp, beam, pre_beam, w, lm, alpha, beta, use_eos=True, lm_on=None, max_steps=None,
           dtype=torch.float64, prefix="decoder.", extra_steps=0):
    """memory (B, T, D) normalised encoder states, mem_len (B,), ctc_logp (B, T, V) log-probabilities or None when w == 0 -> per
    utterance dict(nbest=[(tokens, key, att, ctc, finished, lm)], best, margin, steps, limit, lm_state, n, history=[per step
    dict(tokens (with trailing eos), key, att, ctc, finished, parent, flat, lm_state, lm, n, levels, unk)])."""
    assert 0 <= w <= 1 and 1 <= beam <= pre_beam <= min(64, dcfg.vocab) and lm.vocab_size == dcfg.vocab
    assert (ctc_logp is None) == (w == 0)
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    eos, left = dcfg.vocab - 1, aed_search_ref._left(dcfg, prefix)
    mems = [memory[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]
    xs = [None if w == 0 else ctc_logp[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]

    def logp_of(b):
        return lambda y: aed_ref.decoder_logp(sd, left, dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + list(y), mems[b])[-1]

    limits = [aed_search_ref.limit_of(dcfg, mem_len[b], max_steps) for b in range(len(mems))]
    return search_with(xs, [logp_of(b) for b in range(len(mems))], limits, beam, pre_beam, w, lm, alpha, beta, eos, use_eos, lm_on,
                       extra_steps, dtype)


def recomputed_parts(sd, dcfg, memory, mem_len, ctc_logp, results, w, alpha, beta, lm_on=None, dtype=torch.float32, prefix="decoder."):
    """(key, att, ctc) of the kept candidates of every step of `results`, recomputed in `dtype` without the search: att and ctc
    as aed_joint_ref.recomputed_parts does (w == 0: attention alone, teacher-forced, ctc = 0), the key from them plus the
    rounded LM term of the reference's own (lm, n), which the device must reproduce exactly.  Per utterance, per step, N triples."""
    on = [1] * len(results) if lm_on is None else [int(bool(v)) for v in lm_on]
    if w > 0:
        base = aed_joint_ref.recomputed_parts(sd, dcfg, memory, mem_len, ctc_logp, results, w, dtype=dtype, prefix=prefix)
    else:
        att = aed_search_ref.teacher_forced_scores(sd, dcfg, memory, mem_len, results, dtype=dtype, prefix=prefix)
        base = [[[(-INF if a64 == -INF else a,) * 2 + (0.0,) for a, a64 in zip(row, entry["att"].tolist())]
                 for row, entry in zip(per_step, res["history"])] for per_step, res in zip(att, results)]
    out = []
    for b, (res, per_step) in enumerate(zip(results, base)):
        rows = []
        for entry, row in zip(res["history"], per_step):
            new = []
            for (k, a, c), lm, n in zip(row, entry["lm"], entry["n"]):
                if on[b] and k != -INF:
                    k = float(torch.tensor(k, dtype=dtype) + torch.tensor(lm_term(alpha, beta, lm, n), dtype=dtype))
                new.append((k, a, c))
            rows.append(new)
        out.append(rows)
    return out


e32_of = aed_joint_ref.e32_of
