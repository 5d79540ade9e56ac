"""Host restatement of the WFST search contract of include/m3asr.h ("WFST decoding"), and an exhaustive trellis to check it.

RefSearch follows the contract step by step -- (a) choose, (b) emit, (c) cut, (d) epsilon closure by level -- with numpy
float32 scalars (every add and multiply rounded on its own) and plain dicts; the device search must equal it exactly: words,
word frames, cost bits, reached_final, status.  It also notes which mechanisms decided something (`fired`), so that the test
cases can be shown to exercise them.

trellis() is the check of the restatement: dense Viterbi over every state and frame with no beam, no lists and no levels (the
epsilon arcs are iterated to a fixed point), backtraced through arcs instead of records.
"""
import math

import numpy as np

F = np.float32
NO_ARC = 0xFFFFFFFF
DEAD, TOKEN_CAP, RECORD_CAP, MAX_FRAMES = 1, 2, 4, 8
INF = F(np.inf)


def arc_sources(g):
    return np.repeat(np.arange(g.n_states, dtype=np.int64), np.diff(g.arc_begin.astype(np.int64)))


class RefSearch:
    def __init__(self, g, beam, max_active, acoustic_scale=1.0, token_cap=None, record_cap=None, max_frames=None):
        self.g, self.beam, self.max_active, self.nscale = g, F(beam), int(max_active), F(-F(acoustic_scale))
        self.token_cap = g.n_states if token_cap is None else int(token_cap)
        self.record_cap = 1 << 30 if record_cap is None else int(record_cap)
        self.max_frames = 1 << 30 if max_frames is None else int(max_frames)
        self.src = arc_sources(g)
        self.fired = set()
        self.max_live = 0
        self.reset()

    def reset(self):
        self.records, self.status, self.t = [], 0, 0
        self.cutoff = F(F(0.0) + self.beam)
        nxt = {self.g.start: (F(0.0), NO_ARC)}
        self.cur = self._closure(nxt, {}, 0, self.cutoff, set())
        return self

    def _closure(self, nxt, prev_hist, t, cutoff, had_emit):
        """(d): -> {state: (cost, hist)} of the live states, or None when a capacity was exceeded (status set)."""
        g, hist = self.g, {}
        for L in range(g.n_levels):
            if len(nxt) > self.token_cap:
                self.status |= TOKEN_CAP
                break
            for s in [s for s in nxt if g.eps_level[s] == L]:
                c, arc = nxt[s]
                if not c <= cutoff:
                    self.fired.add("beam")
                    continue
                h = -1
                if arc != NO_ARC:
                    emitting = g.arc_ilabel[arc] != 0
                    h = prev_hist[int(self.src[arc])] if emitting else hist[int(self.src[arc])]
                    if not emitting and s in had_emit:
                        self.fired.add("eps_over_emit")
                    if g.arc_olabel[arc] != 0:
                        self.records.append((h, int(g.arc_olabel[arc]), t))
                        h = len(self.records) - 1
                hist[s] = h
                for a in range(int(g.eps_begin[s]), int(g.arc_begin[s + 1])):
                    cand = F(c + g.arc_weight[a])
                    if not np.isfinite(cand):
                        continue
                    if not cand <= cutoff:
                        self.fired.add("beam")
                        continue
                    d = int(g.arc_dst[a])
                    if d not in nxt or (cand, a) < nxt[d]:
                        nxt[d] = (cand, a)
        else:
            if len(nxt) > self.token_cap:
                self.status |= TOKEN_CAP
        if len(self.records) > self.record_cap:
            self.status |= RECORD_CAP
        if self.status:
            return None
        return {s: (nxt[s][0], hist[s]) for s in nxt if nxt[s][0] <= cutoff}

    def advance(self, logp):
        """logp: (n, V) float32 rows."""
        g = self.g
        for row in np.asarray(logp, dtype=np.float32):
            if self.status:
                return self
            if self.t >= self.max_frames:
                self.status |= MAX_FRAMES
                return self
            self.max_live = max(self.max_live, len(self.cur))
            # (a)
            best = min(c for c, _ in self.cur.values())
            thr = F(best + self.beam)
            exp = sorted((c, s) for s, (c, _) in self.cur.items() if c <= thr)
            if len(exp) < len(self.cur):
                self.fired.add("beam")
            if len(exp) > self.max_active:
                self.fired.add("max_active")
                if exp[self.max_active - 1][0] == exp[self.max_active][0]:
                    self.fired.add("max_active_tie")
                exp = exp[:self.max_active]
            # (b)
            nxt = {}
            for c, s in exp:
                for a in range(int(g.arc_begin[s]), int(g.eps_begin[s])):
                    cand = F(F(c + g.arc_weight[a]) + F(self.nscale * row[g.arc_ilabel[a] - 1]))
                    if not np.isfinite(cand):
                        continue
                    d = int(g.arc_dst[a])
                    if d not in nxt or (cand, a) < nxt[d]:
                        nxt[d] = (cand, a)
            # (c)
            if not nxt:
                self.status |= DEAD
                self.fired.add("dead")
                return self
            cutoff = F(min(c for c, _ in nxt.values()) + self.beam)
            # (d)
            live = self._closure(nxt, {s: h for s, (_, h) in self.cur.items()}, self.t, cutoff, set(nxt))
            if live is None:
                return self
            self.cur, self.cutoff = live, cutoff
            self.t += 1
        return self

    def result(self, final=True):
        """dict(words, frames, n_words, cost, reached_final, status) as the device call reports them."""
        if self.status & ~DEAD:
            return dict(words=[], frames=[], n_words=-1, cost=INF, reached_final=0, status=self.status)
        if self.status:
            return dict(words=[], frames=[], n_words=0, cost=INF, reached_final=0, status=self.status)
        reached, pick = 0, None
        if final:
            cands = [(F(c + self.g.final[s]), s) for s, (c, _) in self.cur.items()]
            cands = [x for x in cands if np.isfinite(x[0])]
            if cands:
                reached, pick = 1, min(cands)
        if pick is None:
            pick = min((c, s) for s, (c, _) in self.cur.items())
        words, frames, h = [], [], self.cur[pick[1]][1]
        while h >= 0:
            h, o, t = self.records[h]
            words.append(o), frames.append(t)
        return dict(words=words[::-1], frames=frames[::-1], n_words=len(words), cost=F(pick[0]), reached_final=reached,
                    status=self.status)


def search(g, logp, beam, max_active, acoustic_scale=1.0, final=True, **caps):
    r = RefSearch(g, beam, max_active, acoustic_scale, **caps).advance(logp)
    return r.result(final), r


def trellis(g, logp, acoustic_scale=1.0):
    """Exhaustive Viterbi (no beam): (best final cost or None, words, frames) by (cost + final, state), ties between arcs to the
    smaller arc id."""
    src = arc_sources(g)
    nscale = F(-F(acoustic_scale))
    eps = [a for a in range(g.n_arcs) if g.arc_ilabel[a] == 0]
    emit = [a for a in range(g.n_arcs) if g.arc_ilabel[a] != 0]

    def close(layer):
        changed = True
        while changed:
            changed = False
            for a in eps:
                s = int(src[a])
                if s in layer:
                    cand = F(layer[s][0] + g.arc_weight[a])
                    d = int(g.arc_dst[a])
                    if np.isfinite(cand) and (d not in layer or (cand, a) < layer[d]):
                        layer[d] = (cand, a)
                        changed = True
        return layer

    layers = [close({g.start: (F(0.0), NO_ARC)})]
    for row in np.asarray(logp, dtype=np.float32):
        prev, layer = layers[-1], {}
        for a in emit:
            s = int(src[a])
            if s in prev:
                cand = F(F(prev[s][0] + g.arc_weight[a]) + F(nscale * row[g.arc_ilabel[a] - 1]))
                d = int(g.arc_dst[a])
                if np.isfinite(cand) and (d not in layer or (cand, a) < layer[d]):
                    layer[d] = (cand, a)
        if not layer:
            return None, [], []
        layers.append(close(layer))
    cands = [(F(c + g.final[s]), s) for s, (c, _) in layers[-1].items()]
    cands = [x for x in cands if np.isfinite(x[0])]
    if not cands:
        return None, [], []
    cost, s = min(cands)
    words, frames, i = [], [], len(layers) - 1
    while True:
        arc = layers[i][s][1]
        if arc == NO_ARC:
            break
        if g.arc_olabel[arc] != 0:
            words.append(int(g.arc_olabel[arc])), frames.append(max(i - 1, 0))
        s = int(src[arc])
        if g.arc_ilabel[arc] != 0:
            i -= 1
    return cost, words[::-1], frames[::-1]


def accepts(g, labels):
    """The smallest cost (float) at which the graph accepts the ilabel sequence `labels` (CTC ids + 1), with the words of one
    such path per final state -- by NFA simulation in float64; None when it does not accept."""
    src = arc_sources(g)

    def close(layer):
        changed = True
        while changed:
            changed = False
            for a in range(g.n_arcs):
                if g.arc_ilabel[a] == 0 and int(src[a]) in layer:
                    c, w = layer[int(src[a])]
                    cand = (c + float(g.arc_weight[a]), w + ((int(g.arc_olabel[a]),) if g.arc_olabel[a] else ()))
                    d = int(g.arc_dst[a])
                    if d not in layer or cand[0] < layer[d][0]:
                        layer[d] = cand
                        changed = True
        return layer

    layer = close({g.start: (0.0, ())})
    for lab in labels:
        nxt = {}
        for a in range(g.n_arcs):
            if g.arc_ilabel[a] == lab and int(src[a]) in layer:
                c, w = layer[int(src[a])]
                cand = (c + float(g.arc_weight[a]), w + ((int(g.arc_olabel[a]),) if g.arc_olabel[a] else ()))
                d = int(g.arc_dst[a])
                if d not in nxt or cand[0] < nxt[d][0]:
                    nxt[d] = cand
        layer = close(nxt)
    fin = [(c + float(g.final[s]), w) for s, (c, w) in layer.items() if math.isfinite(float(g.final[s]))]
    return min(fin) if fin else None
