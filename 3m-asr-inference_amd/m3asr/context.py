"""Hotword biasing of the CTC prefix beam search: phrase lists compiled into the device contract of include/m3asr.h.

The searches (m3_ctc_prefix_beam_search_ctx on the host, m3_ctc_beam_ctx_* on the device) know a weighted deterministic token
automaton -- cls [V], next [n_states][A], delta [n_states][A], pot [n_states] -- and nothing about phrases.  This module
builds those tables from phrases (ContextGraph) and packs graphs into one device image (ContextSet).

    g = ContextGraph([[7, 8, 9], [12, 4]], vocab_size=1434, score=3.0)     # phrases are token-id lists: ids are the interface
    g.walk([7, 8, 9])                                                      # -> (state, bonus, final) = (s, 9.0, 9.0)
    ctx = ContextSet([g], device="cuda")
    search = CtcBeamSearch(B, beam, max_frames, context=ctx)

Semantics, with w = score.  Trie over the phrases; d(s) the depth of state s, end(s) iff a phrase is exactly the path to s.
  pot(root) = 0;  pot(s) = 0 if end(s) else pot(parent) + w        what a partial match has been paid and may have to return
  rew(s) = pot(parent) + w if end(s) else 0                        what completing a phrase keeps
  fail(s)                                                          the Aho-Corasick failure link
  next(s, a) = child of s on a, else next(fail(s), a); at the root the child or the root
  sfx(s) = sum of w d(u) over the end states u on the proper failure chain of s   (phrases ending inside a longer match)
  delta(s, a) = pot(s') - pot(s) + rew(s') + sfx(s'),  s' = next(s, a)
A prefix's bonus is the sum of its arcs' delta (credit token by token, retracted when a partial match fails, kept once the
phrase is complete); final = bonus - pot[state] is the part that is no longer provisional.  When no phrase is a prefix of
another, final = w x (total length of all phrase occurrences in the prefix, overlaps counted).

Limits (checked here and by m3_ctc_context_validate): n_states <= 65536, G <= 1024 graphs, image <= 64 MiB.
"""
from collections import deque

import numpy as np

MAGIC = 0x5843334D
MAX_STATES, MAX_GRAPHS, MAX_BYTES = 65536, 1024, 64 << 20
_HDR_WORDS, _GRAPH_WORDS = 4, 8


def read_phrases(path):
    """A hotword file: one phrase per line as space-separated token ids; empty lines and lines starting with # are skipped."""
    phrases = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            try:
                phrases.append([int(t) for t in line.split()])
            except ValueError:
                raise ValueError("%s:%d: a phrase is a list of token ids, got %r" % (path, n, line))
    return phrases


class ContextGraph:
    """One compiled phrase list: cls (V,) int32, next (n_states, A) int32, delta (n_states, A) float32, pot (n_states,)
    float32.  Column 0 of cls is "in no phrase"; state 0 is the start."""

    def __init__(self, phrases, vocab_size, score=3.0, blank=0):
        V, w = int(vocab_size), float(score)
        if V < 1:
            raise ValueError("ContextGraph: vocab_size = %d < 1" % V)
        if not np.isfinite(w):
            raise ValueError("ContextGraph: score is not finite")
        phrases = [tuple(int(t) for t in p) for p in phrases]
        seen = set()
        for p in phrases:
            if len(p) == 0:
                raise ValueError("ContextGraph: empty phrase")
            if p in seen:
                raise ValueError("ContextGraph: duplicate phrase %r" % (p,))
            seen.add(p)
            for t in p:
                if not 0 <= t < V:
                    raise ValueError("ContextGraph: token %d of phrase %r outside [0, %d)" % (t, p, V))
                if t == blank:
                    raise ValueError("ContextGraph: phrase %r holds the blank id %d" % (p, blank))
        self.phrases, self.vocab_size, self.score, self.blank = phrases, V, w, int(blank)
        # trie
        child, parent, depth, end = [{}], [0], [0], [False]
        for p in phrases:
            s = 0
            for t in p:
                if t not in child[s]:
                    child[s][t] = len(child)
                    child.append({})
                    parent.append(s)
                    depth.append(depth[s] + 1)
                    end.append(False)
                s = child[s][t]
            end[s] = True
        n = len(child)
        if n > MAX_STATES:
            raise ValueError("ContextGraph: %d states > %d" % (n, MAX_STATES))
        tokens = sorted({t for p in phrases for t in p})
        A = len(tokens) + 1
        col = {t: i + 1 for i, t in enumerate(tokens)}
        cls = np.zeros(V, dtype=np.int32)
        for t, c in col.items():
            cls[t] = c
        # states are numbered parent before child, so one pass in index order sees pot(parent) first
        pot, rew = [0.0] * n, [0.0] * n
        for s in range(1, n):
            pot[s] = 0.0 if end[s] else pot[parent[s]] + w
            rew[s] = pot[parent[s]] + w if end[s] else 0.0
        # failure links, the total transition function and sfx, breadth first (a state's link is shallower than the state)
        nxt = np.zeros((n, A), dtype=np.int32)
        fail, sfx = [0] * n, [0.0] * n
        queue = deque()
        for t, s in child[0].items():
            nxt[0, col[t]] = s
            queue.append(s)
        while queue:
            s = queue.popleft()
            f = fail[s]
            sfx[s] = sfx[f] + (w * depth[f] if end[f] else 0.0)
            nxt[s] = nxt[f]
            for t, c in child[s].items():
                nxt[s, col[t]] = c
                fail[c] = int(nxt[f, col[t]])
                queue.append(c)
        potv, rewv, sfxv = (np.asarray(v, dtype=np.float64) for v in (pot, rew, sfx))
        delta = potv[nxt] - potv[:, None] + rewv[nxt] + sfxv[nxt]
        self.n_states, self.A = n, A
        self.cls, self.next = cls, nxt
        self.delta, self.pot = delta.astype(np.float32), potv.astype(np.float32)

    def walk(self, prefix):
        """(state, bonus, final) of a prefix, as the searches compute them: the float32 tables, summed in double left to
        right.  A token outside [0, V) is in no phrase."""
        s, bonus = 0, 0.0
        for t in prefix:
            c = int(self.cls[t]) if 0 <= t < self.vocab_size else 0
            bonus += float(self.delta[s, c])
            s = int(self.next[s, c])
        return s, bonus, bonus - float(self.pot[s])


class ContextSet:
    """G >= 0 graphs over one vocabulary as one image (int32 words, layout in include/m3asr.h), validated by the library
    and, with a device, uploaded.  graph ids are positions in `graphs`; -1 means unbiased."""

    def __init__(self, graphs, device=None, vocab_size=None):
        graphs = list(graphs)
        if len(graphs) > MAX_GRAPHS:
            raise ValueError("ContextSet: %d graphs > %d" % (len(graphs), MAX_GRAPHS))
        if vocab_size is None:
            if not graphs:
                raise ValueError("ContextSet: an empty set needs vocab_size")
            vocab_size = graphs[0].vocab_size
        self.vocab_size = int(vocab_size)
        if any(g.vocab_size != self.vocab_size for g in graphs):
            raise ValueError("ContextSet: the graphs are built for different vocabulary sizes")
        self.graphs = graphs
        self.image = self.pack(graphs, self.vocab_size)
        if self.image.nbytes > MAX_BYTES:
            raise ValueError("ContextSet: image of %d bytes > %d" % (self.image.nbytes, MAX_BYTES))
        from . import ops
        ops.ctc_context_validate(self.image, self.vocab_size)
        self.dev = None
        if device is not None:
            import torch
            self.dev = torch.from_numpy(self.image).to(device)

    def __len__(self):
        return len(self.graphs)

    @staticmethod
    def pack(graphs, vocab_size):
        """The image as a numpy int32 array (not validated)."""
        off = _HDR_WORDS + _GRAPH_WORDS * len(graphs)
        heads, tables = [], []
        for g in graphs:
            head = [g.n_states, g.A]
            for t in (g.cls, g.next, g.delta, g.pot):
                head.append(off)
                tables.append(np.ascontiguousarray(t).reshape(-1).view(np.int32))
                off += tables[-1].size
            heads.append(head + [0, 0])
        words = np.concatenate([np.asarray([MAGIC, len(graphs), vocab_size, off], dtype=np.int64).astype(np.int32),
                                np.asarray(heads, dtype=np.int32).reshape(-1)] + tables)
        assert words.size == off
        return words
