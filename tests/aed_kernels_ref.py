"""Float64-capable mirrors and input builders for the kernel-level tests of the attention decoder (csrc/aed_rescore.hip,
csrc/aed_search.hip): shared by tests/test_aed_kernels_host.py (no GPU: the mirrors against aed_ref / aed_search_ref, the
margin condition of every synthetic case) and tests/test_aed_kernels_gpu.py (the device against the mirrors).  Nothing here is
used by the product, and nothing here launches a kernel.

Every mirror takes its dtype from its inputs: float64 is the truth, the same mirror in float32 on the CPU gives e32, and the
device has to be within max(8 e32, 1e-5) PER OUTPUT ELEMENT (yardstick()).

SYNTHETIC LOGITS.  The search-step cases feed m3_aed_search_prune from tables of logits instead of a decoder.  The values are
multiples of 1/8 in [-4, 4], exact in float32 and float64, so the two precisions cannot disagree on the order of the logits of
a row; candidate scores of different rows differ by the rows' logsumexp and are compared by margin.  Every decision of a case is
either decided by more than twice the bound or is an EXACT tie by construction: equal logits in one row (the lower token id
wins), or bit-identical rows under bit-identical parent scores (the lower flat index wins).  step_margin() tells the two
apart and tests/test_aed_kernels_host.py asserts it for every case."""
import functools
import math

import torch

import aed_search_ref as sref

INF = float("inf")
NAN = float("nan")


def yardstick(ref64, ref32):
    """(e32, bound) of one output: ref64 / ref32 the same mirror in float64 / float32; non-finite elements must agree exactly"""
    a, b = ref64.to(torch.float64), ref32.to(torch.float64)
    fin = torch.isfinite(a)
    assert bool((fin == torch.isfinite(b)).all())
    e32 = float((a[fin] - b[fin]).abs().max()) if bool(fin.any()) else 0.0
    return e32, max(8 * e32, 1e-5)


def max_err(dev, ref64):
    """largest |dev - ref64| over the finite elements of ref64; the others (NaN, -inf) must be the same in dev"""
    a, d = ref64.to(torch.float64), dev.to(torch.float64)
    fin = torch.isfinite(a)
    same = torch.where(torch.isnan(a), torch.isnan(d), d == a)
    assert bool(same[~fin].all()), "a non-finite element of the reference is something else on the device"
    assert bool(torch.isfinite(d[fin]).all()), "a finite element of the reference is not finite on the device"
    return float((a[fin] - d[fin]).abs().max()) if bool(fin.any()) else 0.0


# --------------------------------------------------------------------------------------------------- m3_aed_attention
def _attend(q, K, V, scale):
    """one query (dk,), keys / values (n, dk)"""
    return torch.softmax((K @ q) * scale, dim=0) @ V


def attention(q, k, v, desc, H):
    """include/m3asr.h, m3_aed_attention: q (q_rows, D), k / v (kv_rows, D), desc [(q_row0, n_q, kv_row0, kv_len, causal)]
    -> (out (q_rows, D), zeros where nothing is written; wrote (q_rows,) bool).  A slot with n_q <= 0 does nothing, a slot with
    kv_len <= 0 or a range outside the buffers is skipped."""
    q_rows, D = q.shape
    kv_rows, dk = k.shape[0], D // H
    out = torch.zeros_like(q)
    wrote = torch.zeros(q_rows, dtype=torch.bool)
    scale = 1.0 / math.sqrt(dk)
    for q_row0, n_q, kv_row0, kv_len, causal in desc:
        if n_q <= 0 or kv_len <= 0 or q_row0 < 0 or q_row0 + n_q > q_rows or kv_row0 < 0 or kv_row0 + kv_len > kv_rows:
            continue
        for i in range(n_q):
            n = min(kv_len, i + 1) if causal else kv_len
            for h in range(H):
                c = slice(h * dk, (h + 1) * dk)
                out[q_row0 + i, c] = _attend(q[q_row0 + i, c], k[kv_row0:kv_row0 + n, c], v[kv_row0:kv_row0 + n, c], scale)
            wrote[q_row0 + i] = True
    return out, wrote


# the slots of the rescoring attention case: (n_q, kv_len, causal)
ATT_SLOTS = [(1, 1, 0), (15, 63, 0), (16, 64, 0), (17, 65, 0), (33, 129, 0), (16, 16, 1), (17, 17, 1), (65, 65, 1)]
ATT_MAX_Q = 70                      # larger than every n_q: a fifth query tile that no slot has


@functools.lru_cache(maxsize=None)
def attention_case(H, dk, seed=0):
    """One launch's operands: dict(q, k, v (float32, unused rows NaN), desc, q_rows, kv_rows, max_q, live = slots the mirror
    writes, skipped = {slot: its reserved q rows, which must stay untouched}, twins = [(slot, its copy elsewhere)]).
    Layout of the query rows: 2 reserved rows (the target of the negative q_row0), the live slots with odd gaps, the reserved
    rows of the skip slots, 3 rows at the end for the slot that runs past q_rows."""
    g = torch.Generator().manual_seed(1000 * H + dk + seed)
    D = H * dk
    desc, q_parts, kv_parts = [], [], []
    q_at, kv_at = [2], [3]          # running row counters (lists: closed over)

    def rows(parts, at, n, data=None):
        r0 = at[0]
        parts.append((r0, torch.randn(n, D, generator=g) if data is None else data))
        at[0] += n + 1              # one NaN row between any two ranges
        return r0

    for n_q, kv_len, causal in ATT_SLOTS:
        desc.append([rows(q_parts, q_at, n_q), n_q, rows(kv_parts, kv_at, kv_len), kv_len, causal])
    # a beam sharing its memory: two more slots on the key range of slot 3
    for n_q in (5, 18):
        desc.append([rows(q_parts, q_at, n_q), n_q, desc[3][2], desc[3][3], 0])
    # row independence: slots 3 (non-causal, 17 x 65) and 6 (causal, 17 x 17) again, at other rows and other slot indices
    twins = []
    for src in (3, 6):
        qd = next(d for r0, d in q_parts if r0 == desc[src][0])
        kd = next(d for r0, d in kv_parts if r0 == desc[src][2])
        desc.append([rows(q_parts, q_at, desc[src][1], qd), desc[src][1], rows(kv_parts, kv_at, desc[src][3], kd), desc[src][3],
                     desc[src][4]])
        twins.append((src, len(desc) - 1))
    n_live = len(desc)
    # skip slots, each with query rows of its own that must stay unwritten
    skipped = {}
    r = rows(q_parts, q_at, 4)
    desc.append([r, 0, desc[1][2], 63, 0])                       # n_q = 0
    skipped[len(desc) - 1] = (r, 4)
    r = rows(q_parts, q_at, 4)
    desc.append([r, 4, desc[1][2], 0, 0])                        # kv_len = 0
    skipped[len(desc) - 1] = (r, 4)
    r = rows(q_parts, q_at, 4)
    kv_rows = kv_at[0] + 2
    desc.append([r, 4, kv_rows - 3, 5, 0])                       # kv_row0 + kv_len > kv_rows
    skipped[len(desc) - 1] = (r, 4)
    desc.append([-2, 4, desc[1][2], 63, 0])                      # a negative q_row0: rows 0, 1 are what a clamp would hit
    skipped[len(desc) - 1] = (0, 2)
    q_rows = q_at[0] + 3
    desc.append([q_rows - 3, 5, desc[1][2], 63, 0])              # q_row0 + n_q > q_rows
    skipped[len(desc) - 1] = (q_rows - 3, 3)
    q = torch.full((q_rows, D), NAN)
    k = torch.full((kv_rows, D), NAN)
    for r0, d in q_parts:
        q[r0:r0 + d.shape[0]] = d
    for r0, d in kv_parts:
        k[r0:r0 + d.shape[0]] = d
    v = torch.where(torch.isnan(k), k, torch.randn(kv_rows, D, generator=g))
    for a, b in twins:
        v[desc[b][2]:desc[b][2] + desc[b][3]] = v[desc[a][2]:desc[a][2] + desc[a][3]]
    return dict(q=q, k=k, v=v, desc=desc, q_rows=q_rows, kv_rows=kv_rows, max_q=ATT_MAX_Q, live=list(range(n_live)),
                skipped=skipped, twins=twins, H=H, dk=dk)


@functools.lru_cache(maxsize=None)
def fused_attention_case(H=8, dk=64, seed=5):
    """The driver's layout: one (rows, 3 D) buffer q | k | v, self-attention slots on their own rows plus one non-causal slot"""
    g = torch.Generator().manual_seed(seed)
    D = H * dk
    desc, at = [], 1
    for n in (16, 17, 65):
        desc.append([at, n, at, n, 1])
        at += n + 1
    desc.append([at, 15, desc[2][0], 63, 0])
    rows = at + 15 + 2
    qkv = torch.randn(rows, 3 * D, generator=g)
    return dict(qkv=qkv, desc=desc, rows=rows, max_q=65, H=H, dk=dk)


# ----------------------------------------------------------------------------------------- synthetic logits, search steps
def grid_logits(g, rows, V, lo=-4, hi=4):
    """(rows, V) float32 multiples of 1/8 in [lo, hi]"""
    return torch.randint(lo * 8, hi * 8 + 1, (rows, V), generator=g).to(torch.float32) / 8


def place_eos(row, rank, lift=0.5):
    """in place: the eos logit (last column) gets the given rank among the DISTINCT values of the other logits of the row
    (0 = the largest by `lift`, None = strictly the smallest by a wide gap); midpoints of multiples of 1/8 stay exact"""
    if row.numel() == 1:
        return row
    vals = sorted(set(row[:-1].tolist()), reverse=True)
    if rank is None or rank >= len(vals):
        row[-1] = vals[-1] - 6
    elif rank == 0:
        row[-1] = vals[0] + lift
    else:
        row[-1] = (vals[rank - 1] + vals[rank]) / 2
    return row


def search_limit(mem_len, pe_rows, max_steps):
    return 0 if mem_len < 1 else min(mem_len, pe_rows - 1, max_steps)


def _slot_rows(state, rows):
    """logp_of for aed_search_ref.advance, keyed by slot: advance asks by token list, and the live slots' lists are distinct"""
    live = {}
    for i, (y, f) in enumerate(zip(state["tokens"], state["finished"])):
        if not f and float(state["score"][i]) > -INF:
            assert tuple(y) not in live, "two live slots hold the same tokens"
            live[tuple(y)] = i
    dt = state["score"].dtype
    return lambda y: torch.log_softmax(rows[live[tuple(y)]].to(dt), dim=-1)


def advance_step(state, rows, N, eos):
    """aed_search_ref.frozen_step on the utterance's (N, V) logit rows of this step"""
    return state if state["done"] else sref.advance(state, _slot_rows(state, rows), N, eos)


def nonfinite_step(state, rows, N, eos):
    """The step as include/m3asr.h words it, for the inputs aed_search_ref.advance asserts against (NaN logits, -inf logits,
    fewer than N candidates).  Per unfinished row the N logits that come first in the order (value descending, token id
    ascending), a NaN logit never chosen, candidate = slot score + (logit - logsumexp(row)) in ordinary floating point: a
    -inf slot gives -inf candidates, a row with a NaN has a NaN logsumexp and so NaN candidates; ranks without a logit are
    (-inf, eos).  A finished row offers (score, eos) at rank 0 and (-inf, eos) behind.  Then the N candidates that come first
    in (value descending, flat index slot * N + rank ascending), NaN never chosen; a new slot without a candidate is (-inf,
    eos, parent 0)."""
    if state["done"]:
        return state
    score = state["score"]
    V = rows.shape[1]
    cand = torch.full((N * N,), -INF, dtype=score.dtype)
    tok = [eos] * (N * N)
    for i in range(N):
        if state["finished"][i]:
            cand[i * N] = score[i]
            continue
        x = rows[i].to(score.dtype)
        logp = torch.log_softmax(x, dim=-1)
        order = sorted((c for c in range(V) if not math.isnan(float(x[c]))), key=lambda c: (-float(x[c]), c))[:N]
        for rank, c in enumerate(order):
            cand[i * N + rank] = score[i] + logp[c]
            tok[i * N + rank] = c
    kept = sorted((c for c in range(N * N) if not math.isnan(float(cand[c]))), key=lambda c: (-float(cand[c]), c))[:N]
    kept += [-1] * (N - len(kept))
    parent = [c // N if c >= 0 else 0 for c in kept]
    new_tok = [tok[c] if c >= 0 else eos for c in kept]
    new_score = torch.stack([cand[c] if c >= 0 else cand.new_tensor(-INF) for c in kept])
    tokens = [state["tokens"][p] + [t] for p, t in zip(parent, new_tok)]
    finished = [t == eos for t in new_tok]
    steps = state["steps"] + 1
    entry = dict(tokens=[list(t) for t in tokens], score=new_score.clone(), finished=list(finished), parent=parent)
    return dict(tokens=tokens, score=new_score, finished=finished, steps=steps, limit=state["limit"],
                done=all(finished) or steps >= state["limit"], margin=state["margin"], history=state["history"] + [entry])


def step_margin(state, rows, N, eos):
    """The decision margin of one step of one live utterance, exact ties set apart: pool the candidates of the live slots
    (aed_search_ref, DECISION MARGIN), take the top N + 1 and look at the gaps between neighbours.  A gap of exactly 0 must be a
    tie by construction -- equal logits of one row, or the same token under bit-identical rows and bit-identical parent
    scores -- else it is reported as margin 0.  -> (smallest non-tie gap, number of exact ties)"""
    score, V = state["score"], rows.shape[1]
    vals, slot_of, tok_of = [], [], []
    for i in range(N):
        if state["finished"][i]:
            vals.append(score[i:i + 1])
            slot_of.append(torch.tensor([i]))
            tok_of.append(torch.tensor([eos]))
        elif float(score[i]) > -INF:
            vals.append(score[i] + torch.log_softmax(rows[i].to(score.dtype), dim=-1))
            slot_of.append(torch.full((V,), i))
            tok_of.append(torch.arange(V))
    if not vals:
        return INF, 0
    vals, slot_of, tok_of = torch.cat(vals), torch.cat(slot_of), torch.cat(tok_of)
    fin = torch.isfinite(vals)      # -inf and NaN candidates are told apart by index alone, exactly in any precision
    vals, slot_of, tok_of = vals[fin], slot_of[fin], tok_of[fin]
    top = torch.sort(vals, descending=True, stable=True)[1][:N + 1].tolist()
    margin, ties = INF, 0
    for a, b in zip(top[:-1], top[1:]):
        gap = float(vals[a] - vals[b])
        if gap == 0.0:
            (sa, ta), (sb, tb) = (int(slot_of[a]), int(tok_of[a])), (int(slot_of[b]), int(tok_of[b]))
            fa, fb = state["finished"][sa], state["finished"][sb]
            same_row = sa == sb and not fa and float(rows[sa, ta]) == float(rows[sb, tb])
            twin_rows = (sa != sb and not fa and not fb and ta == tb and torch.equal(rows[sa], rows[sb])
                         and float(score[sa]) == float(score[sb]))
            if same_row or twin_rows:
                ties += 1
                continue
        margin = min(margin, gap)
    return margin, ties


def start_states(case, dtype):
    return [sref.start(case["beam"], search_limit(m, case["pe_rows"], case["reset_steps"]), dtype) for m in case["mem_len"]]


def run_search(case, dtype):
    """-> trace: trace[s][u] = utterance u's state after s prune launches (trace[0] = after reset), a batch in lock step"""
    N, eos = case["beam"], case["V"] - 1
    step = nonfinite_step if case.get("nonfinite") else advance_step
    states = start_states(case, dtype)
    trace = [states]
    for s in range(case["logits"].shape[0]):
        rows = case["logits"][s]
        states = [step(st, rows[u * N:(u + 1) * N], N, eos) for u, st in enumerate(states)]
        trace.append(states)
    return trace


def search_margin(case, trace):
    """(smallest non-tie gap, exact ties) over every step of every live utterance of a trace"""
    N, eos = case["beam"], case["V"] - 1
    margin, ties = INF, 0
    for s in range(case["logits"].shape[0]):
        for u, st in enumerate(trace[s]):
            if not st["done"]:
                m, t = step_margin(st, case["logits"][s][u * N:(u + 1) * N], N, eos)
                margin, ties = min(margin, m), ties + t
    return margin, ties


def final_margin(trace):
    """smallest non-zero gap between the two best final scores (an exact tie gives the first slot); inf for beam 1"""
    margin = INF
    for states in trace:
        for st in states:
            s = sorted(st["score"].tolist(), reverse=True)
            if len(s) > 1 and s[0] != s[1] and s[0] > -INF:
                margin = min(margin, s[0] - s[1])
    return margin


def search_scores(trace):
    """every score of a trace as one tensor (steps + 1, B, N)"""
    return torch.stack([torch.stack([st["score"] for st in states]) for states in trace])


def same_discrete(ta, tb):
    return all(a["tokens"] == b["tokens"] and a["finished"] == b["finished"] and a["steps"] == b["steps"] and a["done"] == b["done"]
               for sa, sb in zip(ta, tb) for a, b in zip(sa, sb))


SEARCH_SHAPES = [(1, 5), (3, 11), (5, 5), (4, 63), (4, 64), (4, 65), (64, 64), (64, 1434)]
SEARCH_MEM = (1, 4, 9)              # B = 3 with unequal limits: 1, 4 and min(9, reset_steps)


@functools.lru_cache(maxsize=None)
def search_case(beam, V, seed=0):
    """B = 3 on synthetic logits.  Descriptor max_steps 12, reset with 7: utterance 0 stops at its limit 1, utterance 1 has
    every slot finished after step 2 (eos far on top in all its rows), before its limit 4, utterance 2 runs into limit 7 with a
    slot that finishes at step 1 (eos on top of one row) and offers (score, eos) alone from then on.  10 launches: 3 more than the
    longest limit, for the frozen check."""
    B, R, steps = 3, 3 * beam, 10
    g = torch.Generator().manual_seed(7919 * beam + V + seed)
    logits = grid_logits(g, steps * R, V).view(steps, R, V)
    for s in range(steps):
        for r in range(R):
            place_eos(logits[s, r], None)
    if V > 1:
        logits[2, beam, -1] = 24.0                                # utterance 1: everybody ends at step 2; ONE row for all its
        logits[2, beam:2 * beam] = logits[2, beam]                # slots, so that equal parent scores stay exact ties
        if beam > 1:
            place_eos(logits[1, 2 * beam], 0, lift=3.0)          # utterance 2, slot 0 (its best) at step 1: kept for sure
    return dict(name="search_%dx%d" % (beam, V), B=B, beam=beam, V=V, mem_len=list(SEARCH_MEM), max_steps=12, reset_steps=7,
                pe_rows=16, logits=logits)


@functools.lru_cache(maxsize=None)
def tie_case():
    """beam 3, V 11, one utterance.  Step 0: tokens 2 and 5 share the largest logit of row 0 -> slot 0 takes token 2, slot 1
    token 5 (the lower token id first), with bit-identical scores.  Step 1: rows 0 and 1 are bit-identical -> their candidates
    tie pairwise and the lower flat index goes first: (slot 0, top), (slot 1, top), (slot 0, second).  The final scores of slots
    0 and 1 are equal and the largest: best = 0, the first slot."""
    beam, V = 3, 11
    g = torch.Generator().manual_seed(31)
    logits = grid_logits(g, 2 * beam, V, lo=-4, hi=0).view(2, beam, V)
    for s in range(2):
        for r in range(beam):
            place_eos(logits[s, r], None)
    logits[0, 0, 2] = logits[0, 0, 5] = 2.0
    logits[0, 0, 7] = 1.0
    logits[1, 0, 4], logits[1, 0, 9] = 3.0, 1.5
    logits[1, 1] = logits[1, 0]
    return dict(name="ties", B=1, beam=beam, V=V, mem_len=[2], max_steps=2, reset_steps=2, pe_rows=8, logits=logits)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """beam 3, V 5, B = 4, two steps, checked against nonfinite_step.
    utterance 0: row 0 holds -inf entries: its third candidate is the -inf logit of the lowest token id, ahead of the -inf
                 candidates of slots 1 and 2 (lower flat index)
    utterance 1: row 0 holds a NaN: NaN logsumexp, nothing of it is chosen; the step-0 slots 1, 2 (score -inf) supply the picks
    utterance 2: step 1 has a row with two non-NaN logits (fewer than beam) and a row of all NaN next to an ordinary row
    utterance 3: ordinary, the neighbour that must not notice"""
    beam, V, B = 3, 5, 4
    g = torch.Generator().manual_seed(77)
    logits = grid_logits(g, 2 * B * beam, V).view(2, B * beam, V)
    for s in range(2):
        for r in range(B * beam):
            place_eos(logits[s, r], None)
    logits[0, 0] = torch.tensor([1.0, -INF, -INF, -INF, 0.5])
    logits[1, 0] = torch.tensor([0.25, -INF, 1.5, -INF, -2.0])
    logits[0, 3] = torch.tensor([1.0, NAN, 0.5, 0.0, -1.0])
    logits[1, 2 * beam + 0] = torch.tensor([NAN, 0.5, NAN, 1.0, NAN])
    logits[1, 2 * beam + 1] = torch.full((V,), NAN)
    return dict(name="nonfinite", B=B, beam=beam, V=V, mem_len=[5, 5, 5, 5], max_steps=3, reset_steps=3, pe_rows=8, logits=logits,
                nonfinite=True)


# ------------------------------------------------------------------------------------------ m3_aed_search_attention
def ancestry(history, s, slot):
    """the slots that wrote key positions 0 .. s of the hypothesis in `slot` at step s (after s prune launches): position s is
    its own, position t < s its ancestor's place at step t, followed through the parents aed_search_ref.advance records"""
    path = [slot]
    for t in range(s - 1, -1, -1):
        path.append(history[t]["parent"][path[-1]])
    return path[::-1]


def search_self_attention(q, kv_steps, histories, s, N, H, utts=None):
    """include/m3asr.h, m3_aed_search_attention, self use at step s: q (R, D); kv_steps[t] (R, 2 D) = the rows' new K | V of step
    t <= s (what the cache holds); histories[u] = the utterance's history.  Row u * N + j attends over positions 0 .. s fetched
    from the slots of ancestry(); utts: the live utterances (default all), the rows of the others stay zero.  -> out (R, D)"""
    R, D = q.shape
    dk = D // H
    out = torch.zeros_like(q)
    for r in range(R):
        u, j = divmod(r, N)
        if utts is not None and u not in utts:
            continue
        rows = [u * N + a for a in ancestry(histories[u], s, j)]
        kv = torch.stack([kv_steps[t][row] for t, row in enumerate(rows)])
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            out[r, c] = _attend(q[r, c], kv[:, c], kv[:, D:][:, c], 1.0 / math.sqrt(dk))
    return out


def search_source_attention(q, kv, mem_row0, mem_len, N, H):
    """source use: row u * N + j attends over memory rows [mem_row0[u], mem_row0[u] + mem_len[u]) of kv (rows, 2 D) = K | V"""
    R, D = q.shape
    dk = D // H
    out = torch.zeros_like(q)
    for r in range(R):
        u = r // N
        m = kv[mem_row0[u]:mem_row0[u] + mem_len[u]]
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            out[r, c] = _attend(q[r, c], m[:, c], m[:, D:][:, c], 1.0 / math.sqrt(dk))
    return out


@functools.lru_cache(maxsize=None)
def walk_case(B, steps, seed=3, mem_len=None, beam=3, V=9):
    """A search that nobody finishes (eos at the bottom of every row), for the self-attention cache: `steps` launches, beam 3,
    random logits so that the picks permute and duplicate parents (tests/test_aed_kernels_host.py asserts that no step of the
    5-step cases, and less than a quarter of the steps of the 70-step cases, has the identity for its parent list)."""
    g = torch.Generator().manual_seed(seed + 17 * B + steps)
    R = B * beam
    logits = grid_logits(g, steps * R, V).view(steps, R, V)
    for s in range(steps):
        for r in range(R):
            place_eos(logits[s, r], None)
    mem_len = [steps] * B if mem_len is None else list(mem_len)
    return dict(name="walk_%d_%d" % (B, steps), B=B, beam=beam, V=V, mem_len=mem_len, max_steps=steps, reset_steps=steps,
                pe_rows=steps + 1, logits=logits)


# ------------------------------------------------------------------------------------------- m3_aed_embed / m3_aed_score
def embed(hyp_tokens, hyp_len, n_hyps, hyp_row0, emb, pe, rows, reverse):
    """include/m3asr.h, m3_aed_embed -> (x (rows, D) zeros where unwritten, target (rows,) int64, wrote (rows,) bool)"""
    B, beam, F = hyp_tokens.shape
    V, D = emb.shape
    x = torch.zeros(rows, D, dtype=emb.dtype)
    target = torch.zeros(rows, dtype=torch.int64)
    wrote = torch.zeros(rows, dtype=torch.bool)
    sos = V - 1
    for h in range(B * beam):
        b, i = divmod(h, beam)
        n, r0, r1 = int(hyp_len[b, i]), int(hyp_row0[h]), int(hyp_row0[h + 1])
        if i >= int(n_hyps[b]):
            continue
        if n < 0 or n > F or n + 1 > pe.shape[0] or r0 < 0 or r1 - r0 != n + 1 or r0 + n + 1 > rows:
            continue
        y = hyp_tokens[b, i, :n].tolist()
        if reverse:
            y = y[::-1]
        for r, tok in enumerate([sos] + y):
            x[r0 + r] = emb[tok] * math.sqrt(D) + pe[r] if 0 <= tok < V else NAN
            target[r0 + r] = y[r] if r < n else sos
            wrote[r0 + r] = True
    return x, target, wrote


def row_logp(logits, target):
    """log_softmax(logits[row])[target[row]], NaN for a target outside [0, V)"""
    V = logits.shape[1]
    lp = torch.log_softmax(logits, dim=-1)
    ok = (target >= 0) & (target < V)
    out = lp.gather(1, target.clamp(0, V - 1).view(-1, 1).long()).view(-1)
    return torch.where(ok, out, torch.full_like(out, NAN))


def score(logits, r_logits, target, r_target, hyp_row0, n_hyps, prior, B, beam, ctc_weight, reverse_weight):
    """include/m3asr.h, m3_aed_score -> (row_logp (2 rows,), att, r_att, final (B, beam), best [B]); the sums run in row order"""
    rows = logits.shape[0]
    dt = logits.dtype
    lp = row_logp(logits, target) if rows else logits.new_zeros(0)
    rlp = row_logp(r_logits, r_target) if (r_logits is not None and rows) else None
    att = torch.full((B, beam), -INF, dtype=dt)
    r_att, final = att.clone(), att.clone()
    best = []
    for b in range(B):
        n = min(max(int(n_hyps[b]), 0), beam)
        for i in range(n):
            r0, r1 = int(hyp_row0[b * beam + i]), int(hyp_row0[b * beam + i + 1])
            if not (r0 >= 0 and r1 > r0 and r1 <= rows):
                continue
            a = lp.new_zeros(())
            for row in range(r0, r1):
                a = a + lp[row]
            f, r = a, lp.new_zeros(())
            if rlp is not None:
                for row in range(r0, r1):
                    r = r + rlp[row]
                f = a * (1 - reverse_weight) + r * reverse_weight
            if ctc_weight != 0:
                f = f + prior[b, i].to(dt) * ctc_weight
            att[b, i], r_att[b, i], final[b, i] = a, r, f
        arg, top = -1, -INF
        for j in range(n):
            if arg < 0 or float(final[b, j]) > top:
                arg, top = j, float(final[b, j])
        best.append(arg)
    return (torch.cat([lp, rlp]) if rlp is not None else lp), att, r_att, final, best
