"""WFST decoding: CTC token-passing beam search over a compiled graph (TLG), on the device (m3_wfst_*).

The token searches (m3asr.decode) rank token prefixes.  A deployed CTC system usually decodes through a graph instead -- a
lexicon composed with a word-level n-gram LM and a CTC token topology -- which is where word LMs, a closed vocabulary,
pronunciation variants and class grammars come from.  This module holds such a graph as the flat image of include/m3asr.h
(DecodingGraph), compiles one from AT&T text (what `fstprint TLG.fst` writes) or from a lexicon, and drives the device search
(CtcWfstSearch).  Everything here is pure Python / numpy; no OpenFst is needed.  Composing a word n-gram G into the graph is
OpenFst's job, offline: print the result with fstprint and read it with from_fst_text.

    graph = DecodingGraph.from_fst_text("TLG.txt", vocab_size=V)             # or .from_lexicon({word id: [token ids]}, V)
    graph.save("TLG.npy"); graph = DecodingGraph.load("TLG.npy").to("cuda")
    search = CtcWfstSearch(graph, B, max_frames, beam=16.0, max_active=7000)
    search.advance(logits_chunk, n_frames)                                   # (B, Tc, V) device logits; chunk after chunk
    search.partial(); search.result()                                        # word ids per utterance
    CtcWfstSearch(graph, B, max_frames, blank_skip=0.98)                     # frames with a sure blank never reach the search

Conventions.  ilabel 0 is epsilon and consumes no frame; ilabel i >= 1 consumes one frame of CTC output id i - 1 (so <blank>
is ilabel 1 when blank is id 0).  olabel 0 is "no output", olabel >= 1 a word id.  Arc and final weights are float32 costs in
the tropical semiring; +inf as a final weight means "not final"; a weight of -0.0 is stored as +0.0.  Arcs are sorted by
(src, emitting before epsilon, ilabel, dst).  eps_level[s] is the length of the longest path of epsilon-input arcs ending in
s.  Limits (checked here and by m3_wfst_validate): no cycle of epsilon-input arcs, n_levels <= 64, n_states <= 2^26, image <=
1 GiB, at least one final state.
"""
import math
import os

import numpy as np

MAGIC, VERSION = 0x5346334D, 1
MAX_STATES, MAX_BYTES, MAX_LEVELS = 1 << 26, 1 << 30, 64
_HDR_WORDS, _TABLES_AT, _WORDS_AT = 20, 8, 16
_TABLES = ("arc_begin", "eps_begin", "arc_ilabel", "arc_olabel", "arc_dst", "arc_weight", "final", "eps_level")
_FLOAT_TABLES = ("arc_weight", "final")
DEAD, TOKEN_CAP, RECORD_CAP, MAX_FRAMES, BAD_GRAPH, WORD_CAP = 1, 2, 4, 8, 16, 32


def read_symbols(path_or_dict):
    """A symbol table: `symbol id` per line (OpenFst's text form), or a dict -> {symbol: id}."""
    if isinstance(path_or_dict, dict):
        return {str(k): int(v) for k, v in path_or_dict.items()}
    syms = {}
    with open(path_or_dict, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `symbol id`, got %r" % (path_or_dict, n, line))
            syms[parts[0]] = int(parts[1])
    return syms


def _eps_levels(n_states, src, dst):
    """eps_level over the epsilon-input arcs (src -> dst); raises on a cycle (naming a state on it) or more than 64 levels."""
    level = np.zeros(n_states, dtype=np.int32)
    if src.size == 0:
        return level
    for _ in range(MAX_LEVELS + 1):
        new = level.copy()
        np.maximum.at(new, dst, level[src] + 1)
        if np.array_equal(new, level):
            return level
        level = new
    # still growing: a cycle, or a chain of more than 64 epsilon arcs.  Peel states without epsilon predecessors.
    indeg = np.bincount(dst, minlength=n_states)
    succ = {}
    for s, d in zip(src.tolist(), dst.tolist()):
        succ.setdefault(s, []).append(d)
    stack = [s for s in range(n_states) if indeg[s] == 0]
    while stack:
        s = stack.pop()
        for d in succ.get(s, ()):
            indeg[d] -= 1
            if indeg[d] == 0:
                stack.append(d)
    left = np.flatnonzero(indeg > 0)
    if left.size == 0:
        raise ValueError("DecodingGraph: n_levels > %d (a chain of more than %d epsilon-input arcs)" % (MAX_LEVELS, MAX_LEVELS - 1))
    pred = {}
    for s, d in zip(src.tolist(), dst.tolist()):
        if indeg[s] > 0 and indeg[d] > 0:
            pred[d] = s
    at = int(left[0])
    for _ in range(left.size):
        at = pred[at]
    raise ValueError("DecodingGraph: the epsilon-input arcs form a cycle through state %d" % at)


class DecodingGraph:
    """A weighted transducer as the tables named in the module text (numpy arrays), `image` (int32 words, layout in
    include/m3asr.h) and, after to(device), `dev`."""

    def __init__(self, n_states, start, src, dst, ilabel, olabel, weight, final, vocab_size):
        """Arcs as five equally long arrays, final as n_states float costs (+inf = not final)."""
        V, N = int(vocab_size), int(n_states)
        if V < 1:
            raise ValueError("DecodingGraph: vocab_size = %d < 1" % V)
        if not 1 <= N <= MAX_STATES:
            raise ValueError("DecodingGraph: n_states = %d outside [1, %d]" % (N, MAX_STATES))
        if not 0 <= int(start) < N:
            raise ValueError("DecodingGraph: start = %d outside [0, %d)" % (start, N))
        src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
        il, ol = np.asarray(ilabel, dtype=np.int64).reshape(-1), np.asarray(olabel, dtype=np.int64).reshape(-1)
        with np.errstate(over="ignore"):
            w = np.asarray(weight, dtype=np.float64).reshape(-1).astype(np.float32)
            fin = np.asarray(final, dtype=np.float64).reshape(-1).astype(np.float32)
        if not (src.size == dst.size == il.size == ol.size == w.size):
            raise ValueError("DecodingGraph: the arc arrays differ in length")
        if fin.size != N:
            raise ValueError("DecodingGraph: %d final weights for %d states" % (fin.size, N))
        for name, a, lo, hi in (("src", src, 0, N - 1), ("dst", dst, 0, N - 1), ("ilabel", il, 0, V), ("olabel", ol, 0, 2 ** 31 - 1)):
            bad = np.flatnonzero((a < lo) | (a > hi))
            if bad.size:
                what = "ilabel > V" if name == "ilabel" and a[bad[0]] > V else name
                raise ValueError("DecodingGraph: arc %d: %s = %d outside [%d, %d]" % (bad[0], what, a[bad[0]], lo, hi))
        if not np.isfinite(w).all():
            raise ValueError("DecodingGraph: arc %d: weight is not finite" % int(np.flatnonzero(~np.isfinite(w))[0]))
        if np.isnan(fin).any() or (fin == -np.inf).any():
            raise ValueError("DecodingGraph: final[%d] is NaN or -inf" % int(np.flatnonzero(np.isnan(fin) | (fin == -np.inf))[0]))
        if not np.isfinite(fin).any():
            raise ValueError("DecodingGraph: no final state")
        w, fin = w + np.float32(0.0), fin + np.float32(0.0)                     # -0.0 + 0.0 = +0.0
        order = np.lexsort((dst, il, il == 0, src))                              # stable: parallel arcs keep their order
        src, dst, il, ol, w = src[order], dst[order], il[order], ol[order], w[order]
        self.vocab_size, self.n_states, self.n_arcs, self.start = V, N, int(src.size), int(start)
        self.arc_begin = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int32)
        self.eps_begin = (self.arc_begin[:-1] + np.bincount(src[il != 0], minlength=N)).astype(np.int32)
        self.arc_ilabel, self.arc_olabel, self.arc_dst = il.astype(np.int32), ol.astype(np.int32), dst.astype(np.int32)
        self.arc_weight, self.final = np.ascontiguousarray(w), np.ascontiguousarray(fin)
        eps = il == 0
        self.eps_level = _eps_levels(N, src[eps], dst[eps])
        self.n_levels = int(self.eps_level.max()) + 1
        if self.n_levels > MAX_LEVELS:
            raise ValueError("DecodingGraph: n_levels = %d > %d" % (self.n_levels, MAX_LEVELS))
        self.image = self.pack()
        self.dev = None

    # ---- compilers
    @classmethod
    def from_fst_text(cls, text_or_path, vocab_size, isymbols=None, osymbols=None):
        """AT&T text, as `fstprint` writes it: arc lines `src dst ilabel olabel [weight]`, final lines `state [weight]`; the
        first line's (source) state is the start state.  Labels are numeric, or symbols of isymbols / osymbols (a `symbol id`
        file or a dict) when those are given."""
        text = text_or_path
        if isinstance(text, os.PathLike) or ("\n" not in text and os.path.exists(text)):
            with open(text, encoding="utf-8") as f:
                text = f.read()
        isym = None if isymbols is None else read_symbols(isymbols)
        osym = None if osymbols is None else read_symbols(osymbols)

        def label(tok, syms, n):
            try:
                return int(syms[tok]) if syms is not None else int(tok)
            except (KeyError, ValueError):
                raise ValueError("fst text line %d: label %r is %s" % (n, tok, "not in the symbol table" if syms is not None else "not a number"))

        src, dst, il, ol, w, finals, start = [], [], [], [], [], {}, None
        for n, line in enumerate(text.splitlines(), 1):
            parts = line.split()
            if not parts:
                continue
            try:
                if len(parts) in (4, 5):
                    s, d = int(parts[0]), int(parts[1])
                    src.append(s), dst.append(d), il.append(label(parts[2], isym, n)), ol.append(label(parts[3], osym, n))
                    w.append(float(parts[4]) if len(parts) == 5 else 0.0)
                elif len(parts) in (1, 2):
                    s = int(parts[0])
                    finals[s] = float(parts[1]) if len(parts) == 2 else 0.0
                else:
                    raise ValueError
            except ValueError as e:
                raise ValueError(str(e) if str(e).startswith("fst text") else "fst text line %d: cannot read %r" % (n, line))
            if start is None:
                start = s
        if start is None:
            raise ValueError("fst text: no states")
        states = src + dst + list(finals)
        if min(states) < 0:
            raise ValueError("fst text: a negative state id")
        N = max(states) + 1
        if N > MAX_STATES:
            raise ValueError("DecodingGraph: n_states = %d outside [1, %d]" % (N, MAX_STATES))
        fin = np.full(N, np.inf, dtype=np.float64)
        for s, f in finals.items():
            fin[s] = f
        return cls(N, start, src, dst, il, ol, w, fin, vocab_size)

    def to_fst_text(self):
        """The graph as AT&T text with numeric labels (every weight written, as its shortest exact decimal)."""
        lines = []
        states = [self.start] + [s for s in range(self.n_states) if s != self.start]
        for s in states:
            for a in range(int(self.arc_begin[s]), int(self.arc_begin[s + 1])):
                lines.append("%d %d %d %d %r" % (s, self.arc_dst[a], self.arc_ilabel[a], self.arc_olabel[a], float(self.arc_weight[a])))
            if np.isfinite(self.final[s]) or (s == self.start and self.arc_begin[s] == self.arc_begin[s + 1]):
                lines.append("%d %r" % (s, float(self.final[s])))
        return "\n".join(lines) + "\n"

    @classmethod
    def from_lexicon(cls, lexicon, vocab_size, blank=0, word_costs=None):
        """The CTC token topology composed with the lexicon, as a free word loop: the graph accepts exactly the CTC alignments
        (blank anywhere, repeats collapse, a blank between two equal adjacent tokens, across a word boundary too) of
        concatenations of zero or more lexicon entries, outputs each word once and charges the sum of the word costs.
        lexicon: {word id >= 1: [token ids]} or {word id: [[token ids], ...]} for several pronunciations.
        word_costs: {word id: cost} (default 0.0 each).

        Shape: a prefix tree of the entries.  Per tree node n two states -- E(n), inside the token of n, and B(n), in blanks
        after it -- E(n) -tok(n)-> E(n), E(n) -blank-> B(n), B(n) -blank-> B(n), and for a child c: B(n) -tok(c)-> E(c), and
        E(n) -tok(c)-> E(c) unless tok(c) = tok(n).  A node that ends a word leaves by epsilon arcs that carry the word and its
        cost: B(n) to the root state R, E(n) to X(tok(n)), the boundary state that remembers the last token.  R -blank-> R,
        R -tok(c)-> E(c) for every first token, X(k) -blank-> R, X(k) -tok(c)-> E(c) unless tok(c) = k.  R is the start; R and
        every X(k) are final."""
        V, blank = int(vocab_size), int(blank)
        if not 0 <= blank < V:
            raise ValueError("from_lexicon: blank = %d outside [0, %d)" % (blank, V))
        children, node_tok, node_words = [{}], [-1], [[]]                        # node 0 is the root
        for word, prons in lexicon.items():
            word = int(word)
            if word < 1:
                raise ValueError("from_lexicon: word id %d < 1" % word)
            prons = list(prons)
            if prons and not isinstance(prons[0], (list, tuple, np.ndarray)):
                prons = [prons]
            if not prons:
                raise ValueError("from_lexicon: word %d has no entry" % word)
            for pron in prons:
                pron = [int(t) for t in pron]
                if not pron:
                    raise ValueError("from_lexicon: word %d has an empty entry" % word)
                n = 0
                for t in pron:
                    if not 0 <= t < V or t == blank:
                        raise ValueError("from_lexicon: token %d of word %d is the blank or outside [0, %d)" % (t, word, V))
                    nxt = children[n].get(t)
                    if nxt is None:
                        nxt = len(children)
                        children[n][t] = nxt
                        children.append({}), node_tok.append(t), node_words.append([])
                    n = nxt
                if word not in node_words[n]:
                    node_words[n].append(word)
        if len(children) == 1:
            raise ValueError("from_lexicon: empty lexicon")
        costs = {} if word_costs is None else {int(k): float(v) for k, v in word_costs.items()}
        n_nodes = len(children)
        end_toks = sorted({node_tok[n] for n in range(1, n_nodes) if node_words[n]})
        # states: R = 0, E(n) = 2 n - 1, B(n) = 2 n (n >= 1), X(k) after them
        X = {k: 2 * n_nodes - 1 + i for i, k in enumerate(end_toks)}
        N = 2 * n_nodes - 1 + len(end_toks)
        bl = blank + 1
        src, dst, il, ol, w = [], [], [], [], []

        def arc(s, d, i, o=0, c=0.0):
            src.append(s), dst.append(d), il.append(i), ol.append(o), w.append(c)

        arc(0, 0, bl)
        for t, c in children[0].items():
            arc(0, 2 * c - 1, t + 1)
        for k, x in X.items():
            arc(x, 0, bl)
            for t, c in children[0].items():
                if t != k:
                    arc(x, 2 * c - 1, t + 1)
        for n in range(1, n_nodes):
            E, Bn, tok = 2 * n - 1, 2 * n, node_tok[n]
            arc(E, E, tok + 1), arc(E, Bn, bl), arc(Bn, Bn, bl)
            for t, c in children[n].items():
                arc(Bn, 2 * c - 1, t + 1)
                if t != tok:
                    arc(E, 2 * c - 1, t + 1)
            for word in node_words[n]:
                arc(E, X[tok], 0, word, costs.get(word, 0.0)), arc(Bn, 0, 0, word, costs.get(word, 0.0))
        fin = np.full(N, np.inf)
        fin[0] = 0.0
        for x in X.values():
            fin[x] = 0.0
        return cls(N, 0, src, dst, il, ol, w, fin, V)

    # ---- the image
    def pack(self):
        """The image as a numpy int32 array (not validated)."""
        head = np.zeros(_HDR_WORDS, dtype=np.int32)
        head[:7] = [MAGIC, VERSION, self.vocab_size, self.n_states, self.n_arcs, self.start, self.n_levels]
        off, tables = _HDR_WORDS, []
        for i, name in enumerate(_TABLES):
            t = np.ascontiguousarray(getattr(self, name))
            assert t.dtype in (np.int32, np.float32)
            head[_TABLES_AT + i] = off
            tables.append(t.view(np.int32))
            off += t.size
        if off * 4 > MAX_BYTES:
            raise ValueError("DecodingGraph: image of %d bytes > %d" % (off * 4, MAX_BYTES))
        head[_WORDS_AT] = off
        return np.concatenate([head] + tables)

    def validate(self):
        from . import ops
        ops.wfst_validate(self.image, self.vocab_size)
        return self

    def save(self, path):
        """The compiled image as .npy."""
        with open(path, "wb") as f:
            np.save(f, self.image)

    @classmethod
    def load(cls, path):
        """An image written by save() (checked by the library before anything is read from it)."""
        image = np.ascontiguousarray(np.load(path, allow_pickle=False))
        if image.dtype != np.int32 or image.ndim != 1 or image.size < _HDR_WORDS or int(image[0]) != MAGIC:
            raise ValueError("%s is not a graph image" % path)
        from . import ops
        ops.wfst_validate(image, int(image[2]))
        return cls._from_image(image)

    @classmethod
    def _from_image(cls, image):
        """The object over an image that the library has validated: the tables are views into it."""
        self = cls.__new__(cls)
        self.image, self.dev = image, None
        self.vocab_size, self.n_states, self.n_arcs, self.start, self.n_levels = (int(v) for v in image[2:7])
        lens = (self.n_states + 1, self.n_states, self.n_arcs, self.n_arcs, self.n_arcs, self.n_arcs, self.n_states, self.n_states)
        for i, (name, ln) in enumerate(zip(_TABLES, lens)):
            t = image[int(image[_TABLES_AT + i]):int(image[_TABLES_AT + i]) + ln]
            setattr(self, name, t.view(np.float32) if name in _FLOAT_TABLES else t)
        return self

    def to(self, device):
        """Upload the image after the library has validated the host copy."""
        import torch
        self.validate()
        self.dev = torch.from_numpy(self.image).to(device)
        return self


def read_lexicon(path, units=None):
    """A lexicon file, `word tok tok ...` per line (a word on several lines has several entries); tokens are ids, or symbols of
    units (a `token id` file or dict) -> (lexicon {word id: [[token ids], ...]}, words [word of id 1, word of id 2, ...])."""
    syms = None if units is None else read_symbols(units)
    lexicon, ids = {}, {}
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 2:
                raise ValueError("%s:%d: expected `word tok tok ...`, got %r" % (path, n, line))
            try:
                toks = [int(syms[t]) if syms is not None else int(t) for t in parts[1:]]
            except (KeyError, ValueError):
                raise ValueError("%s:%d: a token of %r is %s" % (path, n, line, "not in the units" if syms is not None else "not an id"))
            wid = ids.setdefault(parts[0], len(ids) + 1)
            lexicon.setdefault(wid, []).append(toks)
    return lexicon, list(ids)


def read_words(path):
    """A words file, `word id` per line (OpenFst's words.txt) -> {id: word}."""
    return {i: w for w, i in read_symbols(path).items()}


class CtcWfstSearch:
    """B token-passing searches over one graph on the device, resumable at any frame boundary (m3_wfst_search_*).

    beam: a token survives while its cost is within beam of the frame's best (float > 0; math.inf = no beam).  max_active: at
    most that many tokens are expanded per frame, the smallest by (cost, state) exactly.  acoustic_scale multiplies the
    log-probabilities.  token_cap: states touched per frame; record_cap: word-history records between resets; max_frames:
    frames between resets -- exceeding one stops that utterance (result() raises, result_tensors() reports n_words = -1 and
    the status).  max_state_bytes: the constructor refuses a configuration whose device state is larger (24 bytes per graph
    state and utterance, plus the lists).

    blank_skip=p, 0 < p < 1: CTC blank-frame skipping (m3_wfst_skip_*).  A frame whose blank posterior is above
    p is not given to the search (the rule of include/m3asr.h keeps the blank between two equal tokens); the selection runs
    on the device in front of every advance, carries over from chunk to chunk and is reset with the search.  max_frames then
    bounds the DECODED frames between resets, the word frames of result() are still real frame numbers, and frames() tells
    how many frames were seen and decoded.  It is an approximation: costs differ from the unskipped search's and, away from
    peaked posteriors, words may.  blank: the CTC blank id the rule tests.  None (default): no skipping, nothing is allocated
    or launched for it."""

    def __init__(self, graph, B, max_frames, beam=16.0, max_active=7000, acoustic_scale=1.0, token_cap=None, record_cap=None,
                 max_state_bytes=1 << 32, blank_skip=None, blank=0):
        import torch
        from . import _lib, ops
        if graph.dev is None:
            raise _lib.M3Error("CtcWfstSearch: the graph is not on a device (graph.to(device))")
        self.graph, self.device = graph, graph.dev.device
        self.blank_skip, self.skip = None, None
        if blank_skip is not None:
            p = float(blank_skip)
            if not 0.0 < p < 1.0:
                raise _lib.M3Error("CtcWfstSearch: blank_skip = %r outside (0, 1)" % (blank_skip,))
            self.blank_skip = p
            self.log_blank_thresh = float(np.float32(math.log(p)))
            self.skip = ops.wfst_skip_desc(B, graph.vocab_size, blank, max_frames, self.log_blank_thresh)
        N = graph.n_states
        token_cap = min(N, max(65536, 8 * int(max_active))) if token_cap is None else int(token_cap)
        record_cap = (int(max_frames) + 1) * min(N, 2048) if record_cap is None else int(record_cap)
        self.desc = _lib.WfstSearchDesc(int(B), int(max_frames), token_cap, record_cap, int(min(max_active, 2 ** 31 - 1)), N,
                                        graph.n_levels, graph.vocab_size, float(beam), float(acoustic_scale))
        one = _lib.WfstSearchDesc.from_buffer_copy(self.desc)
        one.B = 1
        self.bytes_per_utterance = ops.wfst_search_state_size(one)
        n = self.bytes_per_utterance * int(B)
        if n > int(max_state_bytes):
            raise _lib.M3Error("CtcWfstSearch: %d bytes of device state (%d per utterance, %d graph states) > max_state_bytes = %d"
                               % (n, self.bytes_per_utterance, N, int(max_state_bytes)))
        self.max_words = max(1, min(record_cap, (int(max_frames) + 1) * graph.n_levels))
        self.state = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
        if self.skip is not None:
            self.skip_state = torch.empty(max(ops.wfst_skip_state_size(self.skip), 16), dtype=torch.uint8, device=self.device)
            self.skip_out = torch.empty(0, dtype=torch.float32, device=self.device)     # grown to the largest (Tc + 1) seen
            self.n_kept = torch.zeros(int(B), dtype=torch.int32, device=self.device)
        self.reset()

    @property
    def B(self):
        return self.desc.B

    def reset(self, slots=None):
        """slots: None = all B searches; else the utterances to restart (a list, or an int32 device tensor)."""
        import torch
        from . import ops
        if slots is not None and not torch.is_tensor(slots):
            slots = torch.tensor([int(b) for b in slots], dtype=torch.int32).to(self.device)
        if self.B > 0 and (slots is None or slots.numel() > 0):
            ops.wfst_search_reset(self.desc, self.state, self.graph.dev, slots)
            if self.skip is not None:
                ops.wfst_skip_reset(self.skip, self.skip_state, slots)

    def advance(self, logits_or_logp, n_frames, log_softmax=True):
        """(B, Tc, V) float32 on the device -- logits (log_softmax=True: m3_log_softmax_bias over the rows first) or
        log-probabilities -- and n_frames (B,), the frames of each row that count.  Enqueues without a host sync."""
        import torch
        from . import ops
        x = logits_or_logp
        B, Tc, V = x.shape
        assert B == self.B and V == self.graph.vocab_size, "CtcWfstSearch.advance: (B, Tc, V) = %r for B = %d, V = %d" % (
            tuple(x.shape), self.B, self.graph.vocab_size)
        if Tc == 0 or B == 0:
            return
        nf = n_frames if torch.is_tensor(n_frames) else torch.tensor([int(v) for v in n_frames], dtype=torch.int32)
        nf = nf.reshape(-1).to(self.device, torch.int32, non_blocking=True)
        if log_softmax:
            x = ops.log_softmax_bias(x.contiguous())
        elif not (x.stride(2) == 1 and x.stride(0) == Tc * x.stride(1)):
            x = x.contiguous()
        if self.skip is not None:
            need = B * (Tc + 1) * V
            if self.skip_out.numel() < need:
                self.skip_out = torch.empty(need, dtype=torch.float32, device=self.device)
            kept = self.skip_out[:need].view(B, Tc + 1, V)
            ops.wfst_skip_select(self.skip, self.skip_state, x, nf, kept, self.n_kept)
            x, nf = kept, self.n_kept
        ops.wfst_search_advance(self.desc, self.state, self.graph.dev, x, nf)

    def result_tensors(self, final=True, out=None):
        """(words (B, max_words) -1 padded, frames, n_words (B,), cost (B,), reached_final (B,), status (B,)) on the device.
        With blank_skip the frames are mapped back to real frame numbers (m3_wfst_skip_map_frames)."""
        from . import ops
        out = ops.wfst_search_result(self.desc, self.state, self.graph.dev, final, self.max_words, out)
        if self.skip is not None and self.B > 0:
            ops.wfst_skip_map_frames(self.skip, self.skip_state, out[1], out[2])
        return out

    def frames(self):
        """[(seen, decoded)] per utterance since its reset: the frames advance() was given and those the search took (a search
        with blank_skip; without it the two are equal and nothing counts them: M3Error).  Waits for the device."""
        from . import _lib, ops
        if self.skip is None:
            raise _lib.M3Error("CtcWfstSearch.frames: the search was built without blank_skip")
        if self.B == 0:
            return []
        seen, kept = ops.wfst_skip_counts(self.skip, self.skip_state)
        return list(zip(seen.cpu().tolist(), kept.cpu().tolist()))

    def result(self, final=True, detail=False, slots=None):
        """Word ids per utterance (slots: only the listed utterances, in that order); detail: a dict per utterance with words,
        frames (the frame of each word's record: times the frame shift it is a time), cost, reached_final and status.  Raises
        for a (listed) utterance that overflowed a capacity."""
        from . import _lib
        words, frames, n_words, cost, flags, status = (t.cpu() for t in self.result_tensors(final))
        out = []
        for b in (range(self.B) if slots is None else slots):
            n, st = int(n_words[b]), int(status[b])
            if n < 0:
                why = [name for bit, name in ((TOKEN_CAP, "token_cap = %d" % self.desc.token_cap),
                                              (RECORD_CAP, "record_cap = %d" % self.desc.record_cap),
                                              (MAX_FRAMES, "max_frames = %d" % self.desc.max_frames),
                                              (BAD_GRAPH, "the graph"), (WORD_CAP, "max_words = %d" % self.max_words)) if st & bit]
                raise _lib.M3Error("ctc wfst search: utterance %d exceeded %s (status %d)" % (b, ", ".join(why) or "?", st))
            ws = words[b, :n].tolist()
            out.append(dict(words=ws, frames=frames[b, :n].tolist(), cost=float(cost[b]), reached_final=bool(flags[b]), status=st)
                       if detail else ws)
        return out

    def partial(self):
        """The word ids of each utterance's best live token, final weights aside."""
        return self.result(final=False)


def wfst_from_logits(logits, lens, graph, **kw):
    """logits (B, T', V) on the graph's device, lens (B,) valid frames per utterance -> word ids per utterance (one-shot
    CtcWfstSearch; kw: its options -- blank_skip= / blank= among them -- and detail=)."""
    detail = kw.pop("detail", False)
    B, T = int(logits.shape[0]), int(logits.shape[1])
    search = CtcWfstSearch(graph, B, max(T, 1), **kw)
    search.advance(logits, lens)
    return search.result(detail=detail)
