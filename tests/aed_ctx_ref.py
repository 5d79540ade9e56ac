"""Restatement of attention decoding with hotword biasing, float64-capable (the checker of m3asr.aed_search with context=;
nothing here is used by the product).  THE CONTRACT is everything of tests/aed_lm_ref.py and tests/aed_joint_ref.py (start,
limits, stop rule, max_steps, frozen utterances, stripping, pick order, tie-breaks, the LM's step and term: DESIGN.md 21, 23 and
24), plus the following.  The context graph is m3asr.context's: cls [V], next / delta [n_states][A], pot [n_states].

HYPOTHESIS STATE.  Besides what the searches above carry, a hypothesis carries
    ctx_state  int, a state of its utterance's context graph; 0 for [sos]
    bonus      double, the credit its tokens have collected; 0.0 for [sos]

EXTENDING A LIVE SLOT by candidate c, one of the slot's P = pre_beam largest attention log-probabilities (exactly the picks of
the joint search: the context does not change them):
    c != eos:  col = cls[c], column 0 for a token outside [0, V) or a cls entry outside [0, A);
               bonus' = bonus + (double)delta[ctx_state][col];
               ctx_state' = next[ctx_state][col], state 0 if that entry is outside [0, n_states).  A stored state outside
               [0, n_states) also reads as state 0.
    c == eos:  bonus' = bonus - (double)pot[ctx_state],  ctx_state' = 0.  eos is never walked.  A hypothesis that ends hands back
               the credit of a phrase it never completed; from then on its bonus equals DESIGN.md 15's `final`.

FINISHED SLOTS offer (0, eos) alone and keep key, bonus and ctx_state (and lm, lm_state, n) as they are.

KEY.  key' = jkey + (float)extra,  jkey the joint search's fp32 key (att' when ctc_weight = 0, -inf when a part is).  extra is
evaluated in double as written, without fused multiply-add, and rounded to float32 ONCE:
    (alpha * lm' + beta * n') + bonus'    with an LM that is on for the utterance
    bonus'                                without one
A -inf jkey stays -inf.  The graph's own score is the weight; there is no further multiplier.  (In this restatement jkey is in
the search's dtype; the rounded term is added to it in that dtype.)

PER-UTTERANCE GRAPH.  graph_ids[b] picks the utterance's graph out of a list; -1 or any value outside [0, G) means unbiased:
bonus stays 0.0, ctx_state stays 0, and the utterance's tokens, keys, att, ctc, lm, lm_state and n are those of the same search
without a context, bit for bit (the key gets exactly the LM search's term, or nothing).

PRE-BEAM.  The context is a partial scorer over the pre-beam, like the LM: a row offers P candidates whenever a context is
given, whatever ctc_weight and the LM are.  A hotword token outside a row's P largest attention log-probabilities is not rescued.

AT THE STEP LIMIT.  A hypothesis that reaches max_steps unfinished keeps its provisional credit in its key; the result reports
bonus and ctx_state, and final = bonus - pot[ctx_state] next to them.

eos IN PHRASES.  A graph with cls[V - 1] != 0 is refused (AttentionBeamSearch does; `search` below asserts it).

DECISION MARGIN: the joint search's, over the new keys; the pre-beam gap is kept."""
import numpy as np
import torch

import aed_joint_ref
import aed_lm_ref
import aed_ref
import aed_search_ref

INF = float("inf")


def extra_term(alpha, beta, lm, n, bonus, lm_on, biased):
    """(float)extra as a Python float, or None when nothing is added: Python's doubles do not contract"""
    if lm_on and biased:
        a = float(alpha) * float(lm)
        b = float(beta) * float(n)
        return float(np.float32((a + b) + float(bonus)))
    if lm_on:
        return aed_lm_ref.lm_term(alpha, beta, lm, n)
    if biased:
        return float(np.float32(float(bonus)))
    return None


def ctx_extend(g, state, bonus, c, eos):
    """-> (ctx_state', bonus') of a hypothesis in (state, bonus) extended by c in graph g"""
    st = int(state) if 0 <= int(state) < g.n_states else 0
    if c == eos:
        return 0, bonus - float(g.pot[st])
    col = int(g.cls[c]) if 0 <= c < g.vocab_size else 0
    col = col if 0 <= col < g.A else 0
    nxt = int(g.next[st, col])
    return (nxt if 0 <= nxt < g.n_states else 0), bonus + float(g.delta[st, col])


def start(x, beam, limit, lm, dtype):
    att = torch.full((beam,), -INF, dtype=dtype)
    att[0] = 0
    return dict(tokens=[[] for _ in range(beam)], key=att.clone(), att=att, ctc=torch.zeros(beam, dtype=dtype), finished=[False] * beam,
                states=[aed_joint_ref.initial_state(x) if x is not None else None for _ in range(beam)],
                lm_state=[lm.start if lm is not None else 0] * beam, lm=[0.0] * beam, n=[0] * beam, ctx_state=[0] * beam,
                bonus=[0.0] * beam, steps=0, limit=limit, done=limit < 1, margin=INF, history=[])


def advance(state, x, logp_of, beam, pre_beam, w, lm, alpha, beta, use_eos, lm_on, graph, eos):
    """One step of one live utterance -> the new state (the old one is not touched).  x: the utterance's CTC log-probabilities,
    None exactly when w == 0; lm: None = no LM (lm_on is then 0); graph: the utterance's ContextGraph or None = unbiased."""
    N, P = beam, pre_beam
    dtype = state["att"].dtype
    lm_on = bool(lm_on) and lm is not None
    cands = []          # (flat, key, att, ctc, token, parent, scorer state, lm_state, lm, n, ctx_state, bonus)
    margin = state["margin"]
    for i in range(N):
        if state["finished"][i]:
            cands.append((i * P, state["key"][i].clone(), state["att"][i].clone(), state["ctc"][i].clone(), eos, i, None,
                          state["lm_state"][i], state["lm"][i], state["n"][i], state["ctx_state"][i], state["bonus"][i]))
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
            st2, lm2 = state["lm_state"][i], state["lm"][i]
            cs2, bonus2 = state["ctx_state"][i], state["bonus"][i]
            if lm_on:
                st2, lm2, _, _ = aed_lm_ref.lm_extend(lm, state["lm_state"][i], state["lm"][i], c, eos, use_eos)
            if graph is not None:
                cs2, bonus2 = ctx_extend(graph, state["ctx_state"][i], state["bonus"][i], c, eos)
            key = jkey
            term = extra_term(alpha, beta, lm2, n2, bonus2, lm_on, graph is not None)
            if term is not None and float(jkey) != -INF:
                key = jkey + torch.tensor(term, dtype=dtype)
            cands.append((i * P + k, key, att, psi[k].clone(), c, i, states[k], st2, lm2, n2, cs2, bonus2))
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
               lm_state=[c[7] for c in kept], lm=[c[8] for c in kept], n=[c[9] for c in kept], ctx_state=[c[10] for c in kept],
               bonus=[c[11] for c in kept], steps=state["steps"] + 1, limit=state["limit"])
    entry = dict(tokens=[list(t) for t in tokens], key=new["key"].clone(), att=new["att"].clone(), ctc=new["ctc"].clone(),
                 finished=list(finished), parent=[c[5] for c in kept], flat=[c[0] for c in kept], lm_state=list(new["lm_state"]),
                 lm=list(new["lm"]), n=list(new["n"]), ctx_state=list(new["ctx_state"]), bonus=list(new["bonus"]))
    new.update(done=all(finished) or new["steps"] >= new["limit"], margin=margin, history=state["history"] + [entry])
    return new


def result(state, eos, graph):
    key = state["key"].tolist()
    best = 0
    for i, s in enumerate(key):
        if s > key[best]:
            best = i
    final = [b - (float(graph.pot[s]) if graph is not None else 0.0) for b, s in zip(state["bonus"], state["ctx_state"])]
    nbest = [(aed_search_ref.strip(t, eos), k, a, c, f, l, bo, fi)
             for t, k, a, c, f, l, bo, fi in zip(state["tokens"], key, state["att"].tolist(), state["ctc"].tolist(), state["finished"],
                                                 state["lm"], state["bonus"], final)]
    return dict(nbest=nbest, best=best, margin=state["margin"], steps=state["steps"], limit=state["limit"], history=state["history"],
                states=state["states"], tokens=state["tokens"], lm_state=state["lm_state"], n=state["n"], ctx_state=state["ctx_state"],
                bonus=state["bonus"], final=final)


def graph_of(graphs, graph_ids, B):
    """the ContextGraph (or None = unbiased) of every utterance; graph_ids None: graph 0 for all"""
    ids = [0] * B if graph_ids is None else [int(v) for v in graph_ids]
    assert len(ids) == B
    return [graphs[g] if 0 <= g < len(graphs) else None for g in ids]


def search_with(xs, logp_ofs, limits, beam, pre_beam, w, lm, alpha, beta, eos, graphs, graph_ids=None, use_eos=True, lm_on=None,
                extra_steps=0, dtype=torch.float64):
    """the lock-step loop over utterances given as (x or None, logp_of, limit) triples; a stopped utterance is left alone.
    lm: an NgramLm or None; graphs: a list of ContextGraph (may be empty)"""
    on = [1] * len(limits) if lm_on is None else [int(bool(v)) for v in lm_on]
    gs = graph_of(graphs, graph_ids, len(limits))
    assert len(on) == len(limits) and all((x is None) == (w == 0) for x in xs)
    assert all(int(g.cls[eos]) == 0 for g in graphs), "eos in a phrase"
    states = [start(x, beam, lim, lm, dtype) for x, lim in zip(xs, limits)]
    for _ in range(max(limits) + extra_steps):
        states = [s if s["done"] else advance(s, x, f, beam, pre_beam, w, lm, alpha, beta, use_eos, o, g, eos)
                  for s, x, f, o, g in zip(states, xs, logp_ofs, on, gs)]
    return [result(s, eos, g) for s, g in zip(states, gs)]


def search(sd, dcfg, memory, mem_len, ctc_logp, beam, pre_beam, w, lm, alpha, beta, graphs, graph_ids=None, use_eos=True, lm_on=None,
           max_steps=None, dtype=torch.float64, prefix="decoder.", extra_steps=0):
    """memory (B, T, D) normalised encoder states, mem_len (B,), ctc_logp (B, T, V) log-probabilities or None when w == 0, lm an
    NgramLm or None, graphs a list of ContextGraph -> per utterance dict(nbest=[(tokens, key, att, ctc, finished, lm, bonus,
    final)], best, margin, steps, limit, lm_state, n, ctx_state, bonus, final, history=[per step dict(tokens (with trailing eos),
    key, att, ctc, finished, parent, flat, lm_state, lm, n, ctx_state, bonus)])."""
    assert 0 <= w <= 1 and 1 <= beam <= pre_beam <= min(64, dcfg.vocab) and (lm is None or lm.vocab_size == dcfg.vocab)
    assert (ctc_logp is None) == (w == 0) and all(g.vocab_size == dcfg.vocab for g in graphs)
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    eos, left = dcfg.vocab - 1, aed_search_ref._left(dcfg, prefix)
    mems = [memory[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]
    xs = [None if w == 0 else ctc_logp[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]

    def logp_of(b):
        return lambda y: aed_ref.decoder_logp(sd, left, dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + list(y), mems[b])[-1]

    limits = [aed_search_ref.limit_of(dcfg, mem_len[b], max_steps) for b in range(len(mems))]
    return search_with(xs, [logp_of(b) for b in range(len(mems))], limits, beam, pre_beam, w, lm, alpha, beta, eos, graphs, graph_ids,
                       use_eos, lm_on, extra_steps, dtype)


def recomputed_parts(sd, dcfg, memory, mem_len, ctc_logp, results, w, lm, alpha, beta, graphs, graph_ids=None, lm_on=None,
                     dtype=torch.float32, prefix="decoder."):
    """(key, att, ctc) of the kept candidates of every step of `results`, recomputed in `dtype` without the search: att and ctc
    as aed_lm_ref.recomputed_parts does, the key from them plus the rounded term of the reference's own (lm, n, bonus), which
    the device must reproduce exactly.  Per utterance, per step, N triples."""
    B = len(results)
    on = [0] * B if lm is None else ([1] * B if lm_on is None else [int(bool(v)) for v in lm_on])
    gs = graph_of(graphs, graph_ids, B)
    # the parts without any term: the LM restatement's with every utterance switched off
    base = aed_lm_ref.recomputed_parts(sd, dcfg, memory, mem_len, ctc_logp, results, w, 0.0, 0.0, [0] * B, dtype=dtype, prefix=prefix)
    out = []
    for b, (res, per_step) in enumerate(zip(results, base)):
        rows = []
        for entry, row in zip(res["history"], per_step):
            new = []
            for (k, a, c), lmv, n, bonus in zip(row, entry["lm"], entry["n"], entry["bonus"]):
                term = extra_term(alpha, beta, lmv, n, bonus, on[b], gs[b] is not None)
                if term is not None and k != -INF:
                    k = float(torch.tensor(k, dtype=dtype) + torch.tensor(term, dtype=dtype))
                new.append((k, a, c))
            rows.append(new)
        out.append(rows)
    return out


e32_of = aed_joint_ref.e32_of
