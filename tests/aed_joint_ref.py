"""Restatement of joint CTC/attention decoding in plain torch and numpy, float64-capable (the checker of m3asr.aed_search with
ctc_weight > 0; nothing here is used by the product).  The search is tests/aed_search_ref.py's (start, limits, stop rule,
frozen utterances, result stripping: DESIGN.md 21) with the candidates of every step also scored by the CTC PREFIX probability
of Watanabe et al. 2017, "Hybrid CTC/attention architecture for end-to-end speech recognition", and ranked by the weighted sum.
The reference's own loop is commented out (model/ctc_aed.py keeps only ctc_weight), so this text is the contract.

All quantities are natural logs.  x (m, V): the utterance's CTC log-probabilities, blank = 0, sos = eos = V - 1.
lae(a, b) = max + log(exp(a - max) + exp(b - max)), and -inf when both are -inf (no NaN from -inf - -inf).

SCORER STATE of a hypothesis g (its tokens after sos): rn[t], rb[t], t = 0 .. m-1, the log-probability of the alignments of
x[0..t] that collapse to g and end in non-blank / blank; psi(g).  Start: rn = -inf, rb[t] = x[0][0] + .. + x[t][0], psi = 0.

EXTENSION by candidate c (last = g's last token, none when g is empty):
  c == eos     psi' = lae(rn[m-1], rb[m-1]); the state is not used again
  c == blank   psi' = -inf; the state is all -inf (no alignment collapses to a string that holds a blank, nor to any extension)
  otherwise    s = max(|g|, 1); rn'[s-1] = x[0][c] if g is empty else -inf; rb'[s-1] = -inf; everything below s-1 is -inf;
               phi[t] = rb[t] if c == last else lae(rn[t], rb[t]); psi' = rn'[s-1]; then for t = s .. m-1
                   rn'[t] = lae(rn'[t-1], phi[t-1]) + x[t][c]
                   rb'[t] = lae(rn'[t-1], rb'[t-1]) + x[t][0]
                   psi'   = lae(psi', phi[t-1] + x[t][c])
               (|g| >= m: the loop is empty and psi' = -inf, more tokens than frames)

A SEARCH STEP.  A live slot offers its P largest attention log-probabilities (ties to the lower token id), a finished slot the
single candidate (increment 0, eos, its parts unchanged).  att' = att(g) + logp_att(c | g), ctc' = psi'; the key is
(1 - w) att' + w ctc', and -inf when either part is -inf (so that w = 1 never forms 0 * -inf).  The N largest keys of the
candidates survive, ties to the lower flat index slot * P + rank; -inf keys are legal (dead start slots, blank, more tokens than
frames, a repeated token with no frame left for the blank between) and so order by flat index.  A survivor takes its parent's
tokens and the extended scorer state: one state per hypothesis, copied on prune, nothing recomputed.

DECISION MARGIN, DESIGN.md 21's taken over the keys: per step the smallest gap between consecutive entries among the top N + 1
of the pooled candidates' keys, gaps between two -inf entries not counted (they are exact on both sides); and, because the
pre-beam is a discrete choice of its own, per unfinished slot the gap between its P-th and (P + 1)-th attention log-probability.
The utterance's margin is the minimum over its steps."""
import numpy as np
import torch

import aed_ref
import aed_search_ref

INF = float("inf")


def lae(a, b):
    """on numpy arrays or scalars of one dtype (the scorer's inner loop runs in numpy: the same IEEE arithmetic, less overhead)"""
    with np.errstate(divide="ignore"):
        mx = np.maximum(a, b)
        dead = mx == -INF
        safe = np.where(dead, mx.dtype.type(0), mx)
        out = safe + np.log(np.exp(a - safe) + np.exp(b - safe))
        return np.where(dead, mx.dtype.type(-INF), out)


def _np(x):
    return x.detach().numpy() if isinstance(x, torch.Tensor) else x


def initial_state(x):
    x = _np(x)
    m = x.shape[0]
    rb = np.empty(m, dtype=x.dtype)
    run = x.dtype.type(0)
    for t in range(m):                     # left to right, the order the device's scan keeps
        run = run + x[t, 0]
        rb[t] = run
    return dict(rn=np.full(m, -INF, dtype=x.dtype), rb=rb, n=0, last=None)


def extend(x, state, cands):
    """candidates (token ids) of ONE hypothesis -> (psi' (len(cands),) tensor, [state' per candidate]); a state' of eos is None.
    State arrays are numpy arrays of x's dtype."""
    x = _np(x)
    m, V = x.shape
    eos, n, last = V - 1, state["n"], state["last"]
    rn, rb = state["rn"], state["rb"]
    C = np.asarray(list(cands), dtype=np.int64)
    rn2 = np.full((m, len(cands)), -INF, dtype=x.dtype)
    rb2 = np.full((m, len(cands)), -INF, dtype=x.dtype)
    if n == 0:
        rn2[0] = x[0, C]
    s = max(n, 1)
    psi = rn2[s - 1].copy() if s - 1 < m else np.full(len(cands), -INF, dtype=x.dtype)
    phi_all = lae(rn, rb)
    rep = C == (-1 if last is None else last)
    xc = x[:, C]
    for t in range(s, m):
        phi = np.where(rep, rb[t - 1], phi_all[t - 1])
        rn2[t] = lae(rn2[t - 1], phi) + xc[t]
        rb2[t] = lae(rn2[t - 1], rb2[t - 1]) + x[t, 0]
        psi = lae(psi, phi + xc[t])
    states = []
    for k, c in enumerate(cands):
        if c == eos:
            psi[k] = lae(rn[m - 1], rb[m - 1])
            states.append(None)
        elif c == 0:
            psi[k] = -INF
            states.append(dict(rn=np.full(m, -INF, dtype=x.dtype), rb=np.full(m, -INF, dtype=x.dtype), n=n + 1, last=0))
        else:
            states.append(dict(rn=rn2[:, k].copy(), rb=rb2[:, k].copy(), n=n + 1, last=int(c)))
    return torch.from_numpy(np.ascontiguousarray(psi)), states


def prefix_score(x, tokens):
    """psi of a token list from scratch (an eos ends it): the scorer run over the list, one candidate at a time"""
    state, psi = initial_state(x), torch.zeros((), dtype=x.dtype)
    for c in tokens:
        p, st = extend(x, state, [int(c)])
        psi, state = p[0], st[0]
        if state is None:
            break
    return psi, state


def key_of(att, ctc, w):
    """(1 - w) att + w ctc in the parts' dtype; -inf when a part is"""
    if float(att) == -INF or float(ctc) == -INF:
        return torch.full((), -INF, dtype=att.dtype)
    w = torch.tensor(w, dtype=att.dtype)
    return (1 - w) * att + w * ctc


def start(x, beam, limit):
    dtype = x.dtype
    att = torch.full((beam,), -INF, dtype=dtype)
    att[0] = 0
    key = att.clone()
    return dict(tokens=[[] for _ in range(beam)], key=key, att=att, ctc=torch.zeros(beam, dtype=dtype), finished=[False] * beam,
                states=[initial_state(x) for _ in range(beam)], steps=0, limit=limit, done=limit < 1, margin=INF, history=[])


def advance(state, x, logp_of, beam, pre_beam, w):
    """One step of one live utterance -> the new state (the old one is not touched).  logp_of(tokens) -> (V,) attention
    log-probabilities of the next token after [sos] + tokens."""
    N, P, eos = beam, pre_beam, x.shape[1] - 1
    dtype = x.dtype
    cands = []          # (flat index, key, att, ctc, token, parent, scorer state)
    margin = state["margin"]
    for i in range(N):
        if state["finished"][i]:
            cands.append((i * P, state["key"][i].clone(), state["att"][i].clone(), state["ctc"][i].clone(), eos, i, None))
            continue
        logp = logp_of(state["tokens"][i]).to(dtype)
        order = torch.sort(logp, descending=True, stable=True)[1].tolist()
        top = order[:P]
        if P < len(order):
            margin = min(margin, float(logp[order[P - 1]] - logp[order[P]]))
        psi, states = extend(x, state["states"][i], top)
        for k, c in enumerate(top):
            att = state["att"][i] + logp[c]
            cands.append((i * P + k, key_of(att, psi[k], w), att, psi[k].clone(), c, i, states[k]))
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
               ctc=torch.stack([c[3] for c in kept]), finished=finished, states=[c[6] for c in kept], steps=state["steps"] + 1,
               limit=state["limit"])
    entry = dict(tokens=[list(t) for t in tokens], key=new["key"].clone(), att=new["att"].clone(), ctc=new["ctc"].clone(),
                 finished=list(finished), parent=[c[5] for c in kept], flat=[c[0] for c in kept])
    new.update(done=all(finished) or new["steps"] >= new["limit"], margin=margin, history=state["history"] + [entry])
    return new


def frozen_step(state, x, logp_of, beam, pre_beam, w):
    """the step of an utterance inside a batch: a stopped utterance is left alone"""
    return state if state["done"] else advance(state, x, logp_of, beam, pre_beam, w)


def result(state, eos):
    key = state["key"].tolist()
    best = 0
    for i, s in enumerate(key):
        if s > key[best]:
            best = i
    nbest = [(aed_search_ref.strip(t, eos), k, a, c, f)
             for t, k, a, c, f in zip(state["tokens"], key, state["att"].tolist(), state["ctc"].tolist(), state["finished"])]
    return dict(nbest=nbest, best=best, margin=state["margin"], steps=state["steps"], limit=state["limit"], history=state["history"],
                states=state["states"], tokens=state["tokens"])


def search_with(xs, logp_ofs, limits, beam, pre_beam, w, extra_steps=0):
    """the lock-step loop over utterances given as (x, logp_of, limit) triples"""
    states = [start(x, beam, lim) for x, lim in zip(xs, limits)]
    for _ in range(max(limits) + extra_steps):
        states = [frozen_step(s, x, f, beam, pre_beam, w) for s, x, f in zip(states, xs, logp_ofs)]
    return [result(s, x.shape[1] - 1) for s, x in zip(states, xs)]


def search(sd, dcfg, memory, mem_len, ctc_logp, beam, pre_beam, w, max_steps=None, dtype=torch.float64, prefix="decoder.",
           extra_steps=0):
    """memory (B, T, D) normalised encoder states, mem_len (B,), ctc_logp (B, T, V) log-probabilities -> per utterance
    dict(nbest=[(tokens, key, att, ctc, finished)], best, margin, steps, limit, history=[per step dict(tokens (with trailing
    eos), key, att, ctc, finished, parent, flat)])."""
    assert 0 < w <= 1 and 1 <= beam <= pre_beam <= min(64, dcfg.vocab) and ctc_logp.shape[2] == dcfg.vocab
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    eos, left = dcfg.vocab - 1, aed_search_ref._left(dcfg, prefix)
    mems = [memory[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]
    xs = [ctc_logp[b, :int(mem_len[b])].to(dtype) for b in range(len(mem_len))]

    def logp_of(b):
        return lambda y: aed_ref.decoder_logp(sd, left, dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + list(y), mems[b])[-1]

    limits = [aed_search_ref.limit_of(dcfg, mem_len[b], max_steps) for b in range(len(mems))]
    return search_with(xs, [logp_of(b) for b in range(len(mems))], limits, beam, pre_beam, w, extra_steps)


def _memo_prefix(x, y, memo):
    """prefix_score(x, y), every prefix scored once: the scorer run from scratch, one token at a time"""
    if y not in memo:
        if not y:
            memo[y] = (torch.zeros((), dtype=x.dtype), initial_state(x))
        else:
            p, st = extend(x, _memo_prefix(x, y[:-1], memo)[1], [y[-1]])
            memo[y] = (p[0], st[0])
    return memo[y]


def recomputed_parts(sd, dcfg, memory, mem_len, ctc_logp, results, w, dtype=torch.float32, prefix="decoder."):
    """(key, att, ctc) of the kept candidates of every step of `results`, recomputed in `dtype` without the search: attention
    teacher-forced (aed_search_ref.teacher_forced_scores), the CTC part by the scorer run from scratch over the kept token list,
    the key from the two.  Per utterance, per step, a list of N triples of floats."""
    att = aed_search_ref.teacher_forced_scores(sd, dcfg, memory, mem_len, results, dtype=dtype, prefix=prefix)
    eos = dcfg.vocab - 1
    out = []
    for b, res in enumerate(results):
        x = ctc_logp[b, :int(mem_len[b])].to(dtype)
        memo, per_step = {}, []
        for entry, att_b in zip(res["history"], att[b]):
            row = []
            for toks, a, a64 in zip(entry["tokens"], att_b, entry["att"].tolist()):
                y = list(toks)
                if eos in y:
                    y = y[:y.index(eos) + 1]
                c = _memo_prefix(x, tuple(y), memo)[0]
                a = torch.tensor(-INF if a64 == -INF else a, dtype=dtype)     # a dead start slot: no prefix was ever scored
                row.append((float(key_of(a, c, w)), float(a), float(c)))
            per_step.append(row)
        out.append(per_step)
    return out


def _gap(a, b):
    return 0.0 if a == b else abs(a - b)           # -inf against -inf: exact


def e32_of(results64, parts32):
    """largest |float64 - float32| over key, att and ctc of every kept candidate of every step of every utterance"""
    e = 0.0
    for res, per_step in zip(results64, parts32):
        for entry, row in zip(res["history"], per_step):
            for j, (k, a, c) in enumerate(row):
                e = max(e, _gap(float(entry["key"][j]), k), _gap(float(entry["att"][j]), a), _gap(float(entry["ctc"][j]), c))
    return e
