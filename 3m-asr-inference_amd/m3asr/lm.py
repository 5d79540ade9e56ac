"""N-gram LM shallow fusion of the CTC prefix beam search: ARPA files compiled into the LM image of include/m3asr.h.

The searches (m3_ctc_prefix_beam_search_lm on the host, m3_ctc_beam_lm_* on the device) know a deterministic back-off
automaton over context states and nothing about ARPA files.  This module reads an ARPA file in pure Python / numpy and
builds that automaton (NgramLm), keeps the compiled image as .npy (the compile of a large LM takes minutes), and uploads it.

    lm = NgramLm.from_arpa("lm.arpa", "units.txt")           # units: "token id" lines, a dict, or None (words are ids)
    lm.score([7, 8, 9])                                      # log P(7 8 9 | <s>), natural log, as the searches compute it
    lm.save("lm.npy"); lm = NgramLm.load("lm.npy").to("cuda")
    search = CtcBeamSearch(B, beam, max_frames, lm=lm, lm_weight=0.5, length_bonus=0.0)

States.  State 0 is the empty context; its arcs are dense (uni_logp, uni_next; a token the LM does not know gets unk_logp
and goes to state 0).  A state >= 1 exists for every (n-1)-gram that is the context of some n-gram (and for an n-gram below
the top order that carries a back-off weight without having an extension, so that no weight is lost); states are numbered
shortest context first, so bo_state[s] < s.  A found n-gram leads to the longest suffix of (context + token) that is a
state.  The start state is the <s> context if the LM has one, else 0.

The score contract, step(state, tok):  w = 0.0; st = state; while st != 0: binary-search tok among st's arcs -- found:
return (w + arc_logp, arc_next); else w += bo_weight[st], st = bo_state[st].  At st = 0: (w + uni_logp[tok], uni_next[tok]).
The tables are float32 (the ARPA's log10 values times ln 10 in float64, rounded once); every sum is in double.

N-grams that hold <unk> (other than the unigram), <s> after the first position or </s> before the last are not part of the
automaton and are dropped.  Limits (checked here and by m3_ctc_lm_validate): order <= 8, n_states <= 2^26, image <= 1 GiB.
"""
import math
import os

import numpy as np

MAGIC, VERSION = 0x4D4C334D, 1
MAX_ORDER, MAX_STATES, MAX_BYTES = 8, 1 << 26, 1 << 30
_HDR_WORDS, _TABLES_AT, _WORDS_AT = 20, 8, 17
# an LM set: [SET_MAGIC, SET_VERSION, V, G, words, 0, 0, 0], G x [offset words, n words, scale (float32 bits), 0], the members
SET_MAGIC, SET_VERSION, SET_MAX_MEMBERS, SET_MAX_BYTES = 0x534C334D, 1, 64, 1 << 31
_SET_HDR_WORDS, _SET_ENTRY_WORDS = 8, 4
_TABLES = ("uni_logp", "uni_next", "arc_begin", "arc_tok", "arc_next", "arc_logp", "bo_state", "bo_weight", "final")
BOS, EOS, UNK = -1, -2, -3                         # ids of <s>, </s>, <unk> inside n-gram tuples
_SPECIAL = {"<s>": BOS, "</s>": EOS, "<unk>": UNK}
LN10 = math.log(10.0)


def have_kenlm():
    """Whether kenlm can be imported (it is not needed: the reader below is pure Python)."""
    try:
        import kenlm  # noqa: F401
        return True
    except Exception:
        return False


def read_units(path):
    """A units file: one `token id` pair per line -> {token: id}."""
    units = {}
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `token id`, got %r" % (path, n, line))
            units[parts[0]] = int(parts[1])
    return units


def read_arpa(path_or_text, units=None):
    """-> {n-gram tuple of ids: (log prob, back-off weight)}, natural log, float64.  <s>, </s>, <unk> are BOS, EOS, UNK."""
    text = path_or_text
    if "\n" not in text and not text.lstrip().startswith("\\data\\"):
        with open(text, encoding="utf-8") as f:
            text = f.read()
    if isinstance(units, (str, os.PathLike)):
        units = read_units(units)

    def word_id(w, n):
        if w in _SPECIAL:
            return _SPECIAL[w]
        try:
            return int(units[w]) if units is not None else int(w)
        except (KeyError, ValueError):
            raise ValueError("ARPA line %d: word %r is %s" % (n, w, "not in the units" if units is not None else "not a token id"))

    grams, order, counts, seen_data = {}, 0, {}, False
    for n, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line:
            continue
        if line.startswith("\\"):
            if line == "\\data\\":
                seen_data = True
            elif line == "\\end\\":
                break
            elif line.endswith("-grams:"):
                order = int(line[1:-len("-grams:")])
            else:
                raise ValueError("ARPA line %d: unknown section %r" % (n, line))
            continue
        if not seen_data:
            continue                                            # text in front of \data\ is a comment
        if order == 0:
            if line.startswith("ngram"):
                k, v = line[len("ngram"):].split("=")
                counts[int(k)] = int(v)
                continue
            raise ValueError("ARPA line %d: expected `ngram N=count`, got %r" % (n, line))
        parts = line.split()
        if len(parts) not in (order + 1, order + 2):
            raise ValueError("ARPA line %d: a %d-gram line has %d fields" % (n, order, len(parts)))
        g = tuple(word_id(w, n) for w in parts[1:order + 1])
        if g in grams:
            raise ValueError("ARPA line %d: duplicate n-gram %r" % (n, parts[1:order + 1]))
        grams[g] = (float(parts[0]) * LN10, float(parts[order + 1]) * LN10 if len(parts) == order + 2 else 0.0)
    if not seen_data or not grams:
        raise ValueError("not an ARPA file: no \\data\\ section or no n-grams")
    for k, v in counts.items():
        have = sum(1 for g in grams if len(g) == k)
        if have != v:
            raise ValueError("ARPA: the header promises %d %d-grams, the file has %d" % (v, k, have))
    return grams


class NgramLm:
    """The compiled automaton: the tables named in the module text as numpy arrays, `image` (int32 words, layout in
    include/m3asr.h) and, after to(device), `dev`."""

    def __init__(self, grams, vocab_size, blank=0, unk_logp=math.log(1e-10)):
        """grams: {tuple of ids: (log prob, back-off weight)} in natural log, closed under the prefix rule (every prefix of an
        n-gram is an n-gram); ids are tokens in [0, vocab_size) or BOS / EOS / UNK."""
        V = int(vocab_size)
        if V < 1:
            raise ValueError("NgramLm: vocab_size = %d < 1" % V)
        kept = {}
        for g, (lp, bow) in grams.items():
            g = tuple(int(t) for t in g)
            if len(g) == 0:
                raise ValueError("NgramLm: empty n-gram")
            if not (math.isfinite(lp) and math.isfinite(bow)):
                if g == (BOS,) and math.isfinite(bow):          # some writers give <s> the log prob -inf; it is never predicted
                    lp = -99.0 * LN10
                else:
                    raise ValueError("NgramLm: n-gram %r has a value that is not finite" % (g,))
            if len(g) > 1 and (UNK in g or BOS in g[1:] or EOS in g[:-1]):
                continue
            for t in g:
                if t >= V or t < UNK:
                    raise ValueError("NgramLm: token %d of n-gram %r outside [0, %d)" % (t, g, V))
                if t == blank:
                    raise ValueError("NgramLm: n-gram %r holds the blank id %d" % (g, blank))
            kept[g] = (float(lp), float(bow))
        grams = kept
        if not grams:
            raise ValueError("NgramLm: no n-grams")
        order = max(len(g) for g in grams)
        if order > MAX_ORDER:
            raise ValueError("NgramLm: order %d > %d" % (order, MAX_ORDER))
        for g in grams:
            if len(g) > 1 and g[:-1] not in grams:
                raise ValueError("NgramLm: n-gram %r without its prefix %r" % (g, g[:-1]))
        self.vocab_size, self.order, self.blank = V, order, int(blank)
        self.has_bos, self.has_eos = (BOS,) in grams, (EOS,) in grams
        self.unk_logp = float(np.float32(grams[(UNK,)][0] if (UNK,) in grams else unk_logp))
        if not math.isfinite(self.unk_logp):
            raise ValueError("NgramLm: unk_logp is not finite")
        # states: shortest context first
        ctxs = set()
        for g, (_, bow) in grams.items():
            if len(g) >= 2:
                ctxs.add(g[:-1])
            if bow != 0.0 and len(g) < order and g[-1] != EOS and g != (UNK,):
                ctxs.add(g)
        states = [()] + sorted(ctxs, key=lambda c: (len(c), c))
        n = len(states)
        if n > MAX_STATES:
            raise ValueError("NgramLm: %d states > %d" % (n, MAX_STATES))
        index = {c: i for i, c in enumerate(states)}

        def longest_suffix(g, first):
            for i in range(first, len(g)):
                s = index.get(g[i:])
                if s is not None:
                    return s
            return 0

        bo_state = np.zeros(n, dtype=np.int32)
        bo_weight = np.zeros(n, dtype=np.float64)
        for i, c in enumerate(states[1:], 1):
            bo_state[i] = longest_suffix(c, 1)
            bo_weight[i] = grams[c][1] if c in grams else 0.0
        assert n == 1 or bool((bo_state[1:] < np.arange(1, n)).all())
        # sparse arcs
        a_state, a_tok, a_next, a_logp = [], [], [], []
        for g, (lp, _) in grams.items():
            if len(g) >= 2 and g[-1] >= 0:
                a_state.append(index[g[:-1]])
                a_tok.append(g[-1])
                a_next.append(longest_suffix(g, 0))
                a_logp.append(lp)
        a_state = np.asarray(a_state, dtype=np.int64)
        a_tok = np.asarray(a_tok, dtype=np.int32)
        perm = np.lexsort((a_tok, a_state))
        self.arc_tok = a_tok[perm]
        self.arc_next = np.asarray(a_next, dtype=np.int32)[perm]
        self.arc_logp = np.asarray(a_logp, dtype=np.float64)[perm].astype(np.float32)
        self.arc_begin = np.concatenate([[0], np.cumsum(np.bincount(a_state, minlength=n))]).astype(np.int32)
        # dense arcs of state 0
        self.uni_logp = np.full(V, self.unk_logp, dtype=np.float32)
        self.uni_next = np.zeros(V, dtype=np.int32)
        for g, (lp, _) in grams.items():
            if len(g) == 1 and g[0] >= 0:
                self.uni_logp[g[0]] = lp
                self.uni_next[g[0]] = index.get(g, 0)
        # final: log P(</s> | state), back-off resolved in float64 (bo_state[s] < s: one pass in index order)
        fin = np.zeros(n, dtype=np.float64)
        if self.has_eos:
            fin[0] = grams[(EOS,)][0]
            for i, c in enumerate(states[1:], 1):
                e = grams.get(c + (EOS,))
                fin[i] = e[0] if e is not None else bo_weight[i] + fin[bo_state[i]]
        self.final = fin.astype(np.float32)
        self.bo_state, self.bo_weight = bo_state, bo_weight.astype(np.float32)
        self.n_states, self.n_arcs = n, int(self.arc_tok.size)
        self.start = index.get((BOS,), 0)
        self.n_grams = len(grams)
        self.image = self.pack()
        self.dev = None

    @classmethod
    def from_arpa(cls, path_or_text, units=None, blank=0, vocab_size=None, unk_logp=math.log(1e-10)):
        """units: a `token id` text file, a dict {word: id}, or None = the ARPA's words are decimal token ids.
        vocab_size: default = the largest id of the units (or of the ARPA) + 1."""
        if isinstance(units, (str, os.PathLike)):
            units = read_units(units)
        grams = read_arpa(path_or_text, units)
        if vocab_size is None:
            ids = list(units.values()) if units is not None else [t for g in grams for t in g]
            vocab_size = max([int(t) for t in ids] + [int(blank)]) + 1
        return cls(grams, vocab_size, blank, unk_logp)

    # ---- the score contract in Python
    def step(self, state, tok):
        """(log P(tok | state), next state, back-off levels taken): float32 tables, summed in double."""
        w, st, levels = 0.0, int(state), 0
        while st != 0:
            lo, hi = int(self.arc_begin[st]), int(self.arc_begin[st + 1])
            i = lo + int(np.searchsorted(self.arc_tok[lo:hi], tok))
            if i < hi and int(self.arc_tok[i]) == tok:
                return w + float(self.arc_logp[i]), int(self.arc_next[i]), levels
            w += float(self.bo_weight[st])
            st = int(self.bo_state[st])
            levels += 1
        if 0 <= tok < self.vocab_size:
            return w + float(self.uni_logp[tok]), int(self.uni_next[tok]), levels
        return w + self.unk_logp, 0, levels

    def walk(self, prefix, detail=False):
        """(lm_state, lm) of a prefix from the start state; detail: also the number of back-off levels taken on the way."""
        st, total, levels = self.start, 0.0, 0
        for t in prefix:
            lp, st, lv = self.step(st, int(t))
            total += lp
            levels += lv
        return (st, total, levels) if detail else (st, total)

    def score(self, prefix, eos=False):
        """log P_LM(prefix) (with eos: + log P(</s> | its state)), natural log."""
        st, total = self.walk(prefix)
        return total + (float(self.final[st]) if eos else 0.0)

    # ---- the image
    def pack(self):
        """The image as a numpy int32 array (not validated)."""
        head = np.zeros(_HDR_WORDS, dtype=np.int32)
        head[:7] = [MAGIC, VERSION, self.vocab_size, self.order, self.n_states, self.n_arcs, self.start]
        head[7] = np.float32(self.unk_logp).view(np.int32)
        off, tables = _HDR_WORDS, []
        for i, name in enumerate(_TABLES):
            t = np.ascontiguousarray(getattr(self, name))
            assert t.dtype in (np.int32, np.float32)
            head[_TABLES_AT + i] = off
            tables.append(t.view(np.int32))
            off += t.size
        if off * 4 > MAX_BYTES:
            raise ValueError("NgramLm: image of %d bytes > %d" % (off * 4, MAX_BYTES))
        head[_WORDS_AT] = off
        return np.concatenate([head] + tables)

    def validate(self):
        from . import ops
        ops.ctc_lm_validate(self.image, self.vocab_size)
        return self

    def save(self, path):
        """The compiled image as .npy."""
        with open(path, "wb") as f:
            np.save(f, self.image)

    @classmethod
    def load(cls, path, blank=0):
        """An image written by save() (checked by the library before anything is read from it)."""
        image = np.ascontiguousarray(np.load(path, allow_pickle=False))
        if image.dtype != np.int32 or image.ndim != 1 or image.size < _HDR_WORDS or int(image[0]) != MAGIC:
            raise ValueError("%s is not an LM image" % path)
        from . import ops
        ops.ctc_lm_validate(image, int(image[2]))
        return cls._from_image(image, blank)

    @classmethod
    def _from_image(cls, image, blank=0):
        """The object over an image that the library has validated: the tables are views into it."""
        self = cls.__new__(cls)
        self.image, self.dev, self.blank = image, None, int(blank)
        self.vocab_size, self.order, self.n_states, self.n_arcs, self.start = (int(v) for v in image[2:7])
        self.unk_logp = float(image[7:8].view(np.float32)[0])
        lens = (self.vocab_size, self.vocab_size, self.n_states + 1, self.n_arcs, self.n_arcs, self.n_arcs, self.n_states,
                self.n_states, self.n_states)
        for i, (name, ln) in enumerate(zip(_TABLES, lens)):
            t = image[int(image[_TABLES_AT + i]):int(image[_TABLES_AT + i]) + ln]
            setattr(self, name, t.view(np.float32) if name in ("uni_logp", "arc_logp", "bo_weight", "final") else t)
        self.has_bos, self.has_eos, self.n_grams = self.start != 0, bool(np.any(self.final != 0)), None
        return self

    def to(self, device):
        """Upload the image after the library has validated the host copy."""
        import torch
        self.validate()
        self.dev = torch.from_numpy(self.image).to(device)
        return self


class NgramLmSet:
    """Several NgramLm over one vocabulary in ONE device image (the LM set of include/m3asr.h), so that every utterance of a
    batch, every stream of a pool picks its own: lm_on = j in [1, len(set)] is member j - 1, 0 is "without the LM".  scales[j]
    multiplies the search's lm_weight for member j (in double; 1.0 changes no bit).  The searches take a set wherever they take
    an NgramLm.

        lms = NgramLmSet([general, medical, legal], scales=[1.0, 0.5, 2.0]).to("cuda")
        search = CtcBeamSearch(B, beam, max_frames, lm=lms, lm_weight=0.5)
        search.reset(lm_on=[3, 0, 1, 2])                         # utterance 0: legal, 1: no LM, 2: general, 3: medical
    """

    def __init__(self, lms, scales=None):
        lms = list(lms)
        if not lms:
            raise ValueError("NgramLmSet: no members")
        if len(lms) > SET_MAX_MEMBERS:
            raise ValueError("NgramLmSet: %d members > %d" % (len(lms), SET_MAX_MEMBERS))
        for j, m in enumerate(lms):
            if not isinstance(m, NgramLm):
                raise ValueError("NgramLmSet: member %d is not an NgramLm" % j)
            if m.vocab_size != lms[0].vocab_size:
                raise ValueError("NgramLmSet: member %d is over a vocabulary of %d, member 0 over %d" % (j, m.vocab_size, lms[0].vocab_size))
        scales = [1.0] * len(lms) if scales is None else [float(s) for s in scales]
        if len(scales) != len(lms):
            raise ValueError("NgramLmSet: %d scales for %d members" % (len(scales), len(lms)))
        for j, s in enumerate(scales):
            with np.errstate(over="ignore", under="ignore"):
                s32 = float(np.float32(s)) if math.isfinite(s) else s
            if not (math.isfinite(s32) and s32 > 0.0):
                raise ValueError("NgramLmSet: scale %r of member %d is not finite and positive (as float32)" % (s, j))
        self.lms, self.scales = lms, [float(np.float32(s)) for s in scales]      # the scale the kernels see: the float32
        self.vocab_size, self.blank = lms[0].vocab_size, lms[0].blank
        self.image = self.pack()
        self.dev = None

    def __len__(self):
        return len(self.lms)

    def __getitem__(self, j):
        return self.lms[j]

    def pack(self):
        """The set image as a numpy int32 array (not validated): header, directory, then the members' images, byte for byte,
        each at a multiple of 4 words."""
        G = len(self.lms)
        head = np.zeros(_SET_HDR_WORDS + _SET_ENTRY_WORDS * G, dtype=np.int32)
        off, parts = head.size, []
        for j, (m, s) in enumerate(zip(self.lms, self.scales)):
            pad = -off % 4
            if pad:
                parts.append(np.zeros(pad, dtype=np.int32))
                off += pad
            e = _SET_HDR_WORDS + _SET_ENTRY_WORDS * j
            head[e], head[e + 1] = off, m.image.size
            head[e + 2] = np.float32(s).view(np.int32)
            parts.append(m.image)
            off += m.image.size
        if off * 4 > SET_MAX_BYTES:
            raise ValueError("NgramLmSet: image of %d bytes > %d" % (off * 4, SET_MAX_BYTES))
        head[:5] = [SET_MAGIC, SET_VERSION, self.vocab_size, G, off]
        return np.concatenate([head] + parts)

    def validate(self):
        from . import ops
        ops.ctc_lm_validate(self.image, self.vocab_size)
        return self

    def save(self, path):
        """The set image as .npy."""
        with open(path, "wb") as f:
            np.save(f, self.image)

    @classmethod
    def load(cls, path, blank=0):
        """A set written by save() (checked by the library before anything is read from it)."""
        image = np.ascontiguousarray(np.load(path, allow_pickle=False))
        if image.dtype != np.int32 or image.ndim != 1 or image.size < _SET_HDR_WORDS or int(image[0]) != SET_MAGIC:
            raise ValueError("%s is not an LM set" % path)
        from . import ops
        ops.ctc_lm_validate(image, int(image[2]))
        self = cls.__new__(cls)
        self.image, self.dev, self.blank, self.vocab_size = image, None, int(blank), int(image[2])
        self.lms, self.scales = [], []
        for j in range(int(image[3])):
            e = _SET_HDR_WORDS + _SET_ENTRY_WORDS * j
            self.lms.append(NgramLm._from_image(image[int(image[e]):int(image[e]) + int(image[e + 1])], blank))
            self.scales.append(float(image[e + 2:e + 3].view(np.float32)[0]))
        return self

    def to(self, device):
        """Upload the set (one tensor, .dev) after the library has validated the host copy."""
        import torch
        self.validate()
        self.dev = torch.from_numpy(self.image).to(device)
        return self


def load_lms(specs, units=None, vocab_size=None, use=None):
    """What the command-line tools make of their --lm options: specs, a list of `PATH` or `PATH:SCALE` (an ARPA file, or an
    image saved by NgramLm.save, *.npy), and use, the member --lm-use picks.  One PATH without a scale and without use: a plain
    NgramLm, lm_on None.  Otherwise an NgramLmSet of all of them, and lm_on = use + 1 (use defaults to 0) for every utterance
    of the run.  -> (lm, lm_on), still on the host."""
    if isinstance(specs, str):
        specs = [specs]
    paths, scales = [], []
    for spec in specs:
        path, sep, tail = spec.rpartition(":")
        try:
            scale = float(tail) if sep and path else None
        except ValueError:
            scale = None
        paths.append(spec if scale is None else path)
        scales.append(scale)
    lms = [NgramLm.load(p) if p.endswith(".npy") else NgramLm.from_arpa(p, units, vocab_size=vocab_size) for p in paths]
    if len(lms) == 1 and scales[0] is None and use is None:
        return lms[0], None
    use = 0 if use is None else int(use)
    if not 0 <= use < len(lms):
        raise ValueError("load_lms: use = %d, but %d LM(s) were given" % (use, len(lms)))
    return NgramLmSet(lms, [1.0 if s is None else s for s in scales]), use + 1


def lm_flags(lm, lm_on, n, who, error=ValueError):
    """The lm_on values of a call as n ints.  None: every utterance runs with the LM (a set: with member 0).  A bool or an int
    per utterance: True / 1 = on (a set: member 0), False / 0 = off, j = member j - 1 of a set; a value above len(set) is
    refused here (the kernels would run it as "off", as they run a negative one), and so is a value that is no whole number.
    error: the exception class of the caller's other refusals."""
    if lm_on is None:
        return [1] * n
    vals = lm_on.reshape(-1).tolist() if hasattr(lm_on, "reshape") else list(lm_on)
    if len(vals) != n:
        raise error("%s: lm_on has %d entries for %d utterances" % (who, len(vals), n))
    out = []
    for v in vals:
        if isinstance(lm, NgramLmSet):
            try:
                j = int(v)
                whole = j == v
            except (TypeError, ValueError):
                whole = False
            if not whole:
                raise error("%s: lm_on = %r is not a whole number (0 = off, j = member j - 1)" % (who, v))
            if j > len(lm):
                raise error("%s: lm_on = %r above %d, the set's size (0 = off, j = member j - 1)" % (who, v, len(lm)))
            out.append(max(j, -1))
        else:
            out.append(1 if v else 0)
    return out
