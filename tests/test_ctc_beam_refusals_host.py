"""What the host half of the CTC prefix beam search refuses, and with which words: the return code and the FULL
m3_last_error() text -- or the returned size -- of the fifteen m3_ctc_beam_* / m3_ctc_beam_ctx_* / m3_ctc_beam_lm_* entry points,
called through _lib.load() directly.  The expected strings were taken from a build of the commit before the three families' checks
and launch sites were folded into one call record, one check and three launch functions, and this file passed against that build
unchanged.

No row can reach a kernel launch or a HIP runtime call: in these launchers every refusal comes before the launch and nothing reads
a header back, so made-up aligned pointers are never dereferenced.  Every row is either refused (-2) or returns 0 early through
B == 0, T_chunk == 0 or n == 0; test_calls checks that of an accepted row before it calls.  What is accepted at B > 0 can be
pinned only next to a later refusal (hyp_tokens = NULL with max_frames == 0 in front of a bad image; an absent context image in front of a bad LM image); the
plain family has no refusal behind its pointer check, so its "hyp_tokens may be NULL" is with the GPU tier."""
import ctypes as C

import pytest

from m3asr import _lib

INF, NAN = float("inf"), float("nan")
PTR = 4096              # a made-up aligned address: never dereferenced
BIG = 1 << 20           # bytes of a made-up state that is large enough for every family
CTX_MAX, LMSET_MAX = 64 << 20, 1 << 31
# the smallest descriptor that has all the structure: B = 2, beam = 4, k = 4, max_frames = 8.  Per utterance a 2304-byte slice;
# behind the B slices a 512-byte context block each, behind those a 512-byte LM block each.
PREFIX = {"plain": "ctc_beam", "ctx": "ctc_beam_ctx", "lm": "ctc_beam_lm"}
SIZE = {"plain": 4608, "ctx": 5632, "lm": 6656}
FAMILIES = ("plain", "ctx", "lm")


def desc(B=2, beam=4, k=4, max_frames=8, blank=0):
    return _lib.CtcBeamDesc(B, beam, k, max_frames, blank)


def ref(x):
    return None if x is None else C.byref(x)


BAD_DESC = [
    (None, "ctc_beam: null descriptor"),
    (dict(B=-1), "ctc_beam: B = -1 < 0"),
    (dict(beam=0), "ctc_beam: beam = 0 outside [1, 32]"),
    (dict(beam=33), "ctc_beam: beam = 33 outside [1, 32]"),
    (dict(k=0), "ctc_beam: k = 0 outside [1, 32]"),
    (dict(k=33), "ctc_beam: k = 33 outside [1, 32]"),
    (dict(max_frames=-1), "ctc_beam: max_frames = -1 out of range"),
    (dict(max_frames=1 << 26), "ctc_beam: max_frames = 67108864 out of range"),      # max_frames * beam = 2^28
    (dict(blank=-1), "ctc_beam: blank = -1 < 0"),
]


def mk(kw):
    return None if kw is None else desc(**kw)


# ------------------------------------------------------------------------------------------------------------- 1. the sizes
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kw,msg", BAD_DESC)
def test_sizes_refused(fam, kw, msg):
    assert getattr(_lib.load(), "m3_%s_state_size" % PREFIX[fam])(ref(mk(kw))) == 0
    assert _lib.last_error() == msg


@pytest.mark.parametrize("fam", FAMILIES)
def test_sizes_accepted(fam):
    size = getattr(_lib.load(), "m3_%s_state_size" % PREFIX[fam])
    assert size(C.byref(desc())) == SIZE[fam]
    assert size(C.byref(desc(max_frames=(1 << 26) - 1))) > 0                          # max_frames * beam = 2^28 - 4
    assert size(C.byref(desc(B=0))) == 0


# ----------------------------------------------------------------------------------------------------------- 2. the four calls
# each returns (whether the call returns early when nothing is refused, the export's name, its arguments)
def reset(fam, d, state=PTR, nbytes=BIG):
    return d is not None and d.B == 0, "m3_%s_reset" % PREFIX[fam], [ref(d), state, nbytes, None]


def reset_slots(fam, d, state=PTR, nbytes=BIG, slots=PTR, n=1):
    early = n == 0 or (d is not None and d.B == 0)
    return early, "m3_%s_reset_slots" % PREFIX[fam], [ref(d), state, nbytes, slots, n, None]


def advance(fam, d, state=PTR, nbytes=BIG, image=PTR, image_bytes=64, graph_of=PTR, lm_image=PTR, lm_bytes=80, lm_on=PTR,
            alpha=0.5, beta=0.0, top_logp=PTR, top_idx=PTR, T_chunk=3, n_frames=PTR):
    args = [ref(d), state, nbytes]
    if fam != "plain":
        args += [image, image_bytes, graph_of]
    if fam == "lm":
        args += [lm_image, lm_bytes, lm_on, alpha, beta]
    early = d is not None and (d.B == 0 or T_chunk == 0)
    return early, "m3_%s_advance" % PREFIX[fam], args + [top_logp, top_idx, T_chunk, n_frames, None]


def nbest(fam, d, state=PTR, nbytes=BIG, image=PTR, image_bytes=64, graph_of=PTR, lm_image=PTR, lm_bytes=80, lm_on=PTR,
          alpha=0.5, beta=0.0, use_eos=1, hyp_tokens=PTR, hyp_len=PTR, hyp_score=PTR, hyp_bonus=PTR, hyp_lm=PTR, n_hyps=PTR):
    args = [ref(d), state, nbytes]
    if fam != "plain":
        args += [image, image_bytes, graph_of]
    if fam == "lm":
        args += [lm_image, lm_bytes, lm_on, alpha, beta, use_eos]
    args += [hyp_tokens, hyp_len, hyp_score]
    if fam != "plain":
        args.append(hyp_bonus)
    if fam == "lm":
        args.append(hyp_lm)
    return d is not None and d.B == 0, "m3_%s_nbest" % PREFIX[fam], args + [n_hyps, None]


STATE = "%s: state %d bytes < required %d"
CTX_IMAGE = "%s: image of %d bytes (a multiple of 4 in [16, 67108864])"
LM_IMAGE = "%s: LM image of %d bytes (a multiple of 4 in [80, 2147483648])"
# "everything else null": the state is looked at before the early returns
NO_IMG = dict(state=PTR, image=None, image_bytes=0, graph_of=None, lm_image=None, lm_bytes=0, lm_on=None)
NONE = dict(NO_IMG, top_logp=None, top_idx=None, n_frames=None)
NO_OUT = dict(hyp_tokens=None, hyp_len=None, hyp_score=None, hyp_bonus=None, hyp_lm=None, n_hyps=None)

ROWS = []          # (id, call, kwargs of the descriptor (None = a null one), kwargs of the call, rc, message or None)


def row(fam, call, dkw, kw, rc, msg=None):
    ROWS.append(("%s-%s-%d" % (fam, call.__name__, len(ROWS)), fam, call, dkw, kw, rc, msg))


for fam in FAMILIES:
    p, S = PREFIX[fam], SIZE[fam]
    below = {"plain": None, "ctx": SIZE["plain"], "lm": SIZE["ctx"]}[fam]            # fits the family before, not this one
    has_ctx, has_lm = fam != "plain", fam == "lm"

    # ---- reset and reset_slots.  The message of a bad slot list carries the PLAIN family's name in all three families; the plain
    # family looks at the slot list before the state, the other two at their state first.
    for call in (reset, reset_slots):
        for dkw, msg in (BAD_DESC[0], BAD_DESC[3], BAD_DESC[8]):
            row(fam, call, dkw, {}, -2, msg)
        row(fam, call, {}, dict(state=None), -2, STATE % (p + "_reset", BIG, S))
        row(fam, call, {}, dict(nbytes=S - 1), -2, STATE % (p + "_reset", S - 1, S))
        row(fam, call, {}, dict(nbytes=16), -2, STATE % (p + "_reset", 16, S))
        if below:
            row(fam, call, {}, dict(nbytes=below), -2, STATE % (p + "_reset", below, S))
        row(fam, call, dict(B=0), {}, 0)
        row(fam, call, dict(B=0), dict(nbytes=0), 0)
        row(fam, call, dict(B=0), dict(state=None, nbytes=0), -2, STATE % (p + "_reset", 0, 0))     # also an empty state is non-null
    row(fam, reset_slots, {}, dict(n=-1), -2, "ctc_beam_reset: bad slot list")
    row(fam, reset_slots, dict(B=0), dict(n=-1), -2, "ctc_beam_reset: bad slot list")
    row(fam, reset_slots, {}, dict(n=-1, nbytes=16), -2,
        "ctc_beam_reset: bad slot list" if fam == "plain" else STATE % (p + "_reset", 16, S))
    row(fam, reset_slots, dict(k=33), dict(n=-1), -2, BAD_DESC[5][1])                 # the descriptor before the slot list
    row(fam, reset_slots, {}, dict(slots=None, n=2), -2, p + "_reset_slots: null slot list")
    row(fam, reset_slots, {}, dict(slots=None, n=-1), -2, p + "_reset_slots: null slot list")
    row(fam, reset_slots, None, dict(slots=None, n=2), -2, p + "_reset_slots: null slot list")     # before the descriptor
    row(fam, reset_slots, None, dict(n=0), 0)                                         # n == 0: the descriptor is not looked at
    row(fam, reset_slots, dict(beam=0), dict(state=None, nbytes=0, slots=None, n=0), 0)
    row(fam, reset_slots, {}, dict(nbytes=16, n=0), 0)

    # ---- advance
    for dkw, msg in (BAD_DESC[0], BAD_DESC[1], BAD_DESC[6]):
        row(fam, advance, dkw, {}, -2, msg)
    row(fam, advance, dict(beam=33), dict(T_chunk=0), -2, BAD_DESC[3][1])             # T_chunk == 0 is behind the descriptor
    row(fam, advance, {}, dict(state=None), -2, STATE % (p + "_advance", BIG, S))
    row(fam, advance, {}, dict(nbytes=S - 1), -2, STATE % (p + "_advance", S - 1, S))
    if below:
        row(fam, advance, {}, dict(nbytes=below), -2, STATE % (p + "_advance", below, S))
    row(fam, advance, {}, dict(nbytes=S - 1, top_logp=None), -2, STATE % (p + "_advance", S - 1, S))
    row(fam, advance, {}, dict(nbytes=S - 1, T_chunk=-1), -2, STATE % (p + "_advance", S - 1, S))
    row(fam, advance, {}, dict(nbytes=S - 1, T_chunk=0), -2, STATE % (p + "_advance", S - 1, S))
    row(fam, advance, dict(B=0), dict(state=None, nbytes=0), -2, STATE % (p + "_advance", 0, 0))
    row(fam, advance, {}, dict(T_chunk=-1), -2, p + "_advance: T_chunk = -1 < 0")
    row(fam, advance, dict(B=0), dict(T_chunk=-1), -2, p + "_advance: T_chunk = -1 < 0")
    row(fam, advance, {}, dict(T_chunk=-1, top_idx=None), -2, p + "_advance: T_chunk = -1 < 0")
    row(fam, advance, {}, dict(NONE, T_chunk=0), 0)
    row(fam, advance, {}, dict(NONE, T_chunk=0, nbytes=S), 0)
    row(fam, advance, {}, dict(NONE, T_chunk=0, image_bytes=18, lm_bytes=18, alpha=NAN), 0)
    row(fam, advance, dict(B=0), dict(NONE), 0)
    row(fam, advance, dict(B=0), dict(NONE, nbytes=0, image_bytes=18, lm_bytes=18, beta=INF), 0)
    for name in ("top_logp", "top_idx", "n_frames"):
        row(fam, advance, {}, {name: None}, -2, p + "_advance: null pointer")
    row(fam, advance, {}, dict(n_frames=None, graph_of=None, image_bytes=18, lm_on=None), -2, p + "_advance: null pointer")

    # ---- nbest
    for dkw, msg in (BAD_DESC[0], BAD_DESC[2], BAD_DESC[7]):
        row(fam, nbest, dkw, {}, -2, msg)
    row(fam, nbest, {}, dict(state=None), -2, STATE % (p + "_nbest", BIG, S))
    row(fam, nbest, {}, dict(nbytes=S - 1), -2, STATE % (p + "_nbest", S - 1, S))
    if below:
        row(fam, nbest, {}, dict(nbytes=below), -2, STATE % (p + "_nbest", below, S))
    row(fam, nbest, {}, dict(nbytes=S - 1, hyp_len=None), -2, STATE % (p + "_nbest", S - 1, S))
    row(fam, nbest, dict(B=0), dict(state=None, nbytes=0), -2, STATE % (p + "_nbest", 0, 0))
    row(fam, nbest, dict(B=0), dict(NO_IMG, **NO_OUT), 0)
    row(fam, nbest, dict(B=0), dict(NO_IMG, nbytes=0, image_bytes=18, lm_bytes=18, alpha=INF, **NO_OUT), 0)
    outs = ["hyp_tokens", "hyp_len", "hyp_score", "n_hyps"] + ["hyp_bonus"] * has_ctx + ["hyp_lm"] * has_lm
    for name in outs:
        row(fam, nbest, {}, {name: None}, -2, p + "_nbest: null pointer")
    row(fam, nbest, dict(max_frames=0), dict(hyp_tokens=None, hyp_len=None), -2, p + "_nbest: null pointer")
    row(fam, nbest, {}, dict(n_hyps=None, graph_of=None, image_bytes=18, lm_on=None), -2, p + "_nbest: null pointer")

    # ---- the images, the same rules in advance and nbest (behind the pointers)
    for call in (advance, nbest):
        w = "%s_%s" % (p, call.__name__)
        if has_ctx:
            row(fam, call, {}, dict(graph_of=None), -2, w + ": null graph_of")
            row(fam, call, {}, dict(graph_of=None, image=None), -2, w + ": null graph_of")
            row(fam, call, {}, dict(image=None), -2, w + ": null image of 64 bytes")
            row(fam, call, {}, dict(image=None, image_bytes=18), -2, w + ": null image of 18 bytes")
            for n in (18, 12, 0, CTX_MAX + 4):          # not a multiple of 4, below the header, an image without one, above the maximum
                row(fam, call, {}, dict(image_bytes=n), -2, CTX_IMAGE % (w, n))
            row(fam, call, {}, dict(image=None, image_bytes=0, graph_of=None), -2, w + ": null graph_of")
            row(fam, call, {}, dict(image_bytes=12, lm_bytes=76, lm_on=None, alpha=NAN), -2, CTX_IMAGE % (w, 12))   # context before LM
        if has_lm:
            ok = dict(image=None, image_bytes=0)        # no context image is accepted; the refusal is the LM's
            for base in ({}, ok):
                row(fam, call, {}, dict(base, lm_on=None), -2, w + ": null lm_on")
                row(fam, call, {}, dict(base, lm_on=None, lm_image=None, lm_bytes=82), -2, w + ": null lm_on")
                row(fam, call, {}, dict(base, lm_image=None), -2, w + ": null LM image of 80 bytes")
                row(fam, call, {}, dict(base, lm_image=None, lm_bytes=82, alpha=NAN), -2, w + ": null LM image of 82 bytes")
                for n in (82, 76, 0, LMSET_MAX + 4):
                    row(fam, call, {}, dict(base, lm_bytes=n), -2, LM_IMAGE % (w, n))
                row(fam, call, {}, dict(base, lm_bytes=76, beta=INF), -2, LM_IMAGE % (w, 76))
                for ab in (dict(alpha=NAN), dict(alpha=INF), dict(beta=NAN), dict(beta=-INF)):
                    row(fam, call, {}, dict(base, **ab), -2, w + ": alpha or beta is not finite")
                row(fam, call, {}, dict(base, lm_image=None, lm_bytes=0, alpha=NAN), -2, w + ": alpha or beta is not finite")
    # hyp_tokens may be NULL when max_frames == 0: the refusal is the image's, not the pointers'
    if has_ctx:
        row(fam, nbest, dict(max_frames=0), dict(hyp_tokens=None, image_bytes=18), -2, CTX_IMAGE % (p + "_nbest", 18))
    if has_lm:
        row(fam, nbest, dict(max_frames=0), dict(hyp_tokens=None, lm_bytes=76), -2, LM_IMAGE % (p + "_nbest", 76))


@pytest.mark.parametrize("fam,call,dkw,kw,rc,msg", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_calls(fam, call, dkw, kw, rc, msg):
    assert rc in (0, -2) and (msg is None) == (rc == 0)
    early, name, args = call(fam, mk(dkw), **kw)
    assert rc == -2 or early, "a row that is accepted must return through B == 0, T_chunk == 0 or n == 0"
    assert getattr(_lib.load(), name)(*args) == rc
    if msg is not None:
        assert _lib.last_error() == msg
