"""What the host half of csrc/aed_joint.hip refuses, and with which words: the return code and the FULL
m3_last_error() text -- or the returned size -- of the m3_aed_joint_* / m3_aed_ngram_* / m3_aed_bias_* entry points, called through
_lib.load() directly.  The expected strings were taken from a build of the commit before the three families' checks and launch
sites were folded into one call record, one check and one launch table, and this file passed against that build unchanged.

No row can reach a kernel launch or a HIP runtime call:
  1. the six *_state_size / *_scratch_size functions are host arithmetic over a descriptor;
  2. score / prune / result (and m3_aed_joint_reset) get a B = 0 descriptor, NULL or made-up 16-byte aligned pointers: every one
     of them returns before its launch;
  3. the three resets that read an image header back get only rows refused BEFORE that read: a bad descriptor, a short or
     misaligned state at B > 0, an image size out of range.
The rules that bite only at B > 0 with real blobs (size shortfalls, "exactly when", "together", null graph_of) are with the
test_refusals functions of the GPU tier."""
import ctypes as C

import pytest

from m3asr import _lib

INF, NAN = float("inf"), float("nan")
PTR = 4096              # a made-up 16-byte aligned address: never dereferenced
ODD = 4104              # ... and one that is not 16-byte aligned
LM_MAX, LMSET_MAX, CTX_MAX = 1 << 30, 1 << 31, 64 << 20


def desc(B=3, beam=3, max_steps=9, V=11, pre_beam=5, max_frames=64):
    return _lib.AedJointDesc(_lib.AedSearchDesc(B, beam, max_steps, V, 32, 2, 2, 100), pre_beam, max_frames)


def bias(image=PTR, image_bytes=64, graph_of=None, state=None, state_bytes=0, scratch=None, scratch_bytes=0):
    b = _lib.AedBias()
    b.image, b.image_bytes, b.graph_of = image, image_bytes, graph_of
    b.state, b.state_bytes, b.scratch, b.scratch_bytes = state, state_bytes, scratch, scratch_bytes
    return b


def ref(x):
    return None if x is None else C.byref(x)


def up(n):
    return 256 * -(-n // 256)


# ------------------------------------------------------------------------------------------------------------- 1. the sizes
PRE_BEAM = "%s: pre_beam = %d, need beam = 3 <= pre_beam <= min(64, V = 11)"
BIG = dict(B=65535, beam=64, max_steps=1, V=64, pre_beam=64)     # the most rows and candidates the search's descriptor allows
SIZE_ROWS = []
for fam, prefix in (("joint", "aed_joint"), ("ngram", "aed_ngram"), ("bias", "aed_ngram")):   # the bias family asks the LM's check
    for p in (2, 65, 12):                                         # below beam, above 64, above V
        SIZE_ROWS.append((fam, dict(pre_beam=p), PRE_BEAM % (prefix, p)))
    SIZE_ROWS.append((fam, dict(beam=1, V=1, pre_beam=1),
                      "%s: V = 1, %s and eos need two different ids" % (prefix, "blank" if fam == "joint" else "a token")))
    # an overflow that every family reports in the search's words, because the search's own check comes first
    SIZE_ROWS.append((fam, dict(B=65535, beam=64, max_steps=1 << 16, V=64, pre_beam=64),
                      "aed_search: 4194240 rows of 65536 steps overflow the int32 state offsets"))
    SIZE_ROWS.append((fam, None, "aed_%s: null descriptor" % fam))
SIZE_ROWS += [
    ("joint", dict(max_frames=0), "aed_joint: max_frames = 0 outside [1, 2^20]"),
    ("joint", dict(max_frames=(1 << 20) + 1), "aed_joint: max_frames = 1048577 outside [1, 2^20]"),
    ("joint", dict(B=1024, beam=64, V=100, pre_beam=64, max_frames=1 << 20),
     "aed_joint: 65536 rows of 1048576 frames overflow the int32 offsets of the scorer state"),
    ("joint", dict(B=1, beam=64, V=100, pre_beam=64, max_frames=1 << 20),
     "aed_joint: 64 rows x 64 candidates x 1048576 frames overflow the int32 offsets of the candidate scratch"),
]


@pytest.mark.parametrize("fam,kw,msg", SIZE_ROWS)
def test_sizes_refused(fam, kw, msg):
    lib = _lib.load()
    d = None if kw is None else desc(**kw)
    for which in ("state", "scratch"):
        assert getattr(lib, "m3_aed_%s_%s_size" % (fam, which))(ref(d)) == 0
        assert _lib.last_error() == msg


def test_sizes_accepted():
    """B * beam rows, K = pre_beam candidates, F frames: the formulas of the blob layouts.  The LM and context families do not
    look at max_frames.  Their own overflow rules (rows * 16 words, rows * K * 8 words against 2^31 - 1) cannot fire: at the most
    the search's descriptor allows, B = 65535 and beam = pre_beam = 64, the larger product is 2147450880, and that shape is
    accepted."""
    lib = _lib.load()
    R, K, F = 9, 5, 64
    d = desc()
    assert lib.m3_aed_joint_state_size(C.byref(d)) == up(4 * R * 2 * (4 + 2 * F))
    assert lib.m3_aed_joint_scratch_size(C.byref(d)) == up(4 * R * K * (4 + 2 * F))
    for F2 in (64, 0, (1 << 20) + 1):
        d = desc(max_frames=F2)
        assert lib.m3_aed_ngram_state_size(C.byref(d)) == up(4 * R * 2 * 8)
        assert lib.m3_aed_ngram_scratch_size(C.byref(d)) == up(4 * R * K * 8)
        assert lib.m3_aed_bias_state_size(C.byref(d)) == up(4 * R * 2 * 4)
        assert lib.m3_aed_bias_scratch_size(C.byref(d)) == up(4 * R * K * 8)
    d, R, K = desc(max_frames=0, **BIG), 65535 * 64, 64
    assert R * K * 8 == 2147450880 < 2 ** 31 - 1
    assert lib.m3_aed_ngram_state_size(C.byref(d)) == up(4 * R * 2 * 8) and lib.m3_aed_ngram_scratch_size(C.byref(d)) == up(4 * R * K * 8)
    assert lib.m3_aed_bias_state_size(C.byref(d)) == up(4 * R * 2 * 4) and lib.m3_aed_bias_scratch_size(C.byref(d)) == up(4 * R * K * 8)


# ------------------------------------------------------------------------------- 2. score, prune, result with B = 0 descriptors
def joint_score(d, ldl=11, ldc=11, ctc_rows=0, w=0.3):
    return _lib.load().m3_aed_joint_score(ref(d), None, 0, None, 0, None, 0, None, ldl, None, ldc, ctc_rows, w, None)


def joint_reset(d, ldc=11, ctc_rows=0):
    return _lib.load().m3_aed_joint_reset(ref(d), None, 0, None, 0, None, ldc, ctc_rows, None)


def joint_prune(d):
    return _lib.load().m3_aed_joint_prune(ref(d), None, 0, None, 0, None, 0, None, None)


def joint_result(d):
    return _lib.load().m3_aed_joint_result(ref(d), None, 0, None, 0, None, None, None)


def ngram_score(d, ldl=11, ldc=11, ctc_rows=0, w=0.0, lm_bytes=80, alpha=0.5, beta=0.0, use_eos=1):
    return _lib.load().m3_aed_ngram_score(ref(d), None, 0, None, 0, None, 0, None, 0, None, 0, None, ldl, None, ldc, ctc_rows, w, None,
                                          lm_bytes, None, alpha, beta, use_eos, None)


def ngram_prune(d, jstate=None):
    return _lib.load().m3_aed_ngram_prune(ref(d), None, 0, jstate, 0, None, 0, None, 0, None, 0, None, None)


def ngram_result(d):
    return _lib.load().m3_aed_ngram_result(ref(d), None, 0, None, 0, None, None, None, None, None)


def bias_score(d, b, ldl=11, ldc=11, ctc_rows=0, w=0.0, lm_image=None, lm_bytes=0, lstate=None, alpha=0.0, beta=0.0, use_eos=1):
    return _lib.load().m3_aed_bias_score(ref(d), None, 0, None, 0, None, 0, lstate, 0, None, 0, None, ldl, None, ldc, ctc_rows, w, lm_image,
                                         lm_bytes, None, alpha, beta, use_eos, ref(b), None)


def bias_prune(d, b, lscratch=None):
    return _lib.load().m3_aed_bias_prune(ref(d), None, 0, None, 0, None, 0, None, 0, lscratch, 0, ref(b), None, None)


def bias_result(d, b):
    return _lib.load().m3_aed_bias_result(ref(d), None, 0, ref(b), None, None, None, None)


E = dict(B=0)                                                     # the empty batch: every entry returns before its launch
LM_IMAGE = "%s: LM image of %d bytes (a multiple of 4 in [80, %d])"
CTX_IMAGE = "%s: context image of %d bytes (a multiple of 4 in [16, 67108864])"
LM_BLOB = "%s: an LM blob without the other (LM state and LM scratch are NULL exactly when there is no LM)"
EMPTY_ROWS = [
    # ---- m3_aed_joint_*: ctc_weight in (0, 1]
    (lambda: joint_score(desc(**E)), 0, None),
    (lambda: joint_score(desc(**E), w=1.0), 0, None),
    (lambda: joint_score(desc(**E), w=0.0), -2, "aed_joint_score: ctc_weight = 0 outside (0, 1] (0 is m3_aed_search_prune)"),
    (lambda: joint_score(desc(**E), w=1.5), -2, "aed_joint_score: ctc_weight = 1.5 outside (0, 1] (0 is m3_aed_search_prune)"),
    (lambda: joint_score(desc(**E), w=NAN), -2, "aed_joint_score: ctc_weight = nan outside (0, 1] (0 is m3_aed_search_prune)"),
    (lambda: joint_score(desc(**E), ldl=10, w=0.0), -2, "aed_joint_score: ldl = 10 < V = 11"),           # before the weight
    (lambda: joint_score(desc(**E), ldc=10, ldl=10), -2, "aed_joint_score: ldc = 10 < V = 11"),          # before ldl
    (lambda: joint_score(desc(**E), ctc_rows=-1), -2, "aed_joint_score: ctc_rows = -1"),
    (lambda: joint_score(desc(max_frames=0, **E)), -2, "aed_joint: max_frames = 0 outside [1, 2^20]"),
    (lambda: joint_score(None), -2, "aed_joint: null descriptor"),
    (lambda: joint_reset(desc(**E)), 0, None),
    (lambda: joint_reset(desc(**E), ldc=10, ctc_rows=-1), -2, "aed_joint_reset: ldc = 10 < V = 11"),
    (lambda: joint_reset(desc(**E), ctc_rows=-1), -2, "aed_joint_reset: ctc_rows = -1"),
    (lambda: joint_prune(desc(**E)), 0, None),
    (lambda: joint_prune(desc(pre_beam=2, **E)), -2, PRE_BEAM % ("aed_joint", 2)),
    (lambda: joint_result(desc(**E)), 0, None),
    (lambda: joint_result(desc(pre_beam=65, **E)), -2, PRE_BEAM % ("aed_joint", 65)),
    # ---- m3_aed_ngram_*: ctc_weight in [0, 1]; without CTC max_frames is not looked at, with it the joint family's words
    (lambda: ngram_score(desc(max_frames=0, **E)), 0, None),
    (lambda: ngram_score(desc(**E), w=0.3), 0, None),
    (lambda: ngram_score(desc(**E), w=1.0), 0, None),
    (lambda: ngram_score(None, w=-0.5), -2, "aed_ngram_score: ctc_weight = -0.5 outside [0, 1]"),      # before the descriptor
    (lambda: ngram_score(desc(**E), w=1.5), -2, "aed_ngram_score: ctc_weight = 1.5 outside [0, 1]"),
    (lambda: ngram_score(None), -2, "aed_ngram: null descriptor"),
    (lambda: ngram_score(desc(max_frames=0, **E), w=0.3), -2, "aed_joint: max_frames = 0 outside [1, 2^20]"),
    (lambda: ngram_score(desc(pre_beam=2, **E), w=0.3), -2, PRE_BEAM % ("aed_joint", 2)),
    (lambda: ngram_score(desc(pre_beam=2, **E)), -2, PRE_BEAM % ("aed_ngram", 2)),
    (lambda: ngram_score(desc(**E), ldc=10, w=0.3), -2, "aed_ngram_score: ldc = 10 < V = 11"),
    (lambda: ngram_score(desc(**E), ldc=10), 0, None),                                                  # no CTC: ldc is not looked at
    (lambda: ngram_score(desc(**E), ctc_rows=-1, w=0.3), -2, "aed_ngram_score: ctc_rows = -1"),
    (lambda: ngram_score(desc(**E), ldl=10, lm_bytes=82), -2, "aed_ngram_score: ldl = 10 < V = 11"),   # before the image
    (lambda: ngram_score(desc(**E), lm_bytes=82, alpha=INF), -2, LM_IMAGE % ("aed_ngram_score", 82, LMSET_MAX)),
    (lambda: ngram_score(desc(**E), lm_bytes=76), -2, LM_IMAGE % ("aed_ngram_score", 76, LMSET_MAX)),
    (lambda: ngram_score(desc(**E), lm_bytes=LMSET_MAX + 4), -2, LM_IMAGE % ("aed_ngram_score", LMSET_MAX + 4, LMSET_MAX)),
    (lambda: ngram_score(desc(**E), alpha=INF, use_eos=2), -2, "aed_ngram_score: alpha or beta is not finite"),
    (lambda: ngram_score(desc(**E), beta=NAN), -2, "aed_ngram_score: alpha or beta is not finite"),
    (lambda: ngram_score(desc(**E), use_eos=2), -2, "aed_ngram_score: use_eos = 2"),
    (lambda: ngram_prune(desc(max_frames=0, **E)), 0, None),
    (lambda: ngram_prune(desc(**E), jstate=PTR), 0, None),                                              # a scorer state: the CTC form
    (lambda: ngram_prune(desc(max_frames=0, **E), jstate=PTR), -2, "aed_joint: max_frames = 0 outside [1, 2^20]"),
    (lambda: ngram_prune(None), -2, "aed_ngram: null descriptor"),
    (lambda: ngram_result(desc(max_frames=0, **E)), 0, None),
    (lambda: ngram_result(desc(beam=1, V=1, pre_beam=1, **E)), -2, "aed_ngram: V = 1, a token and eos need two different ids"),
    # ---- m3_aed_bias_*: ctc_weight in [0, 1]; the LM part is optional
    (lambda: bias_score(desc(max_frames=0, **E), bias()), 0, None),
    (lambda: bias_score(desc(**E), bias(), w=0.3), 0, None),
    (lambda: bias_score(desc(**E), bias(), w=0.3, lm_image=PTR, lm_bytes=80, alpha=0.5), 0, None),
    (lambda: bias_score(desc(max_frames=0, **E), bias(), lm_image=PTR, lm_bytes=80), 0, None),
    (lambda: bias_score(None, None, w=1.5), -2, "aed_bias_score: ctc_weight = 1.5 outside [0, 1]"),
    (lambda: bias_score(desc(**E), bias(), w=-0.5), -2, "aed_bias_score: ctc_weight = -0.5 outside [0, 1]"),
    (lambda: bias_score(None, bias()), -2, "aed_bias: null descriptor"),
    (lambda: bias_score(desc(max_frames=0, **E), bias(), w=0.3), -2, "aed_joint: max_frames = 0 outside [1, 2^20]"),
    (lambda: bias_score(desc(pre_beam=12, **E), bias()), -2, PRE_BEAM % ("aed_ngram", 12)),
    (lambda: bias_score(desc(**E), None, ldl=10), -2, "aed_bias_score: null bias record"),             # before ldl
    (lambda: bias_score(desc(**E), bias(), lstate=PTR), -2, LM_BLOB % "aed_bias_score"),                # before the bias record
    (lambda: bias_score(desc(**E), bias(image_bytes=12)), -2, CTX_IMAGE % ("aed_bias_score", 12)),
    (lambda: bias_score(desc(**E), bias(image_bytes=18)), -2, CTX_IMAGE % ("aed_bias_score", 18)),
    (lambda: bias_score(desc(**E), bias(image_bytes=CTX_MAX + 4)), -2, CTX_IMAGE % ("aed_bias_score", CTX_MAX + 4)),
    (lambda: bias_score(desc(**E), bias(image=None)), -2, CTX_IMAGE % ("aed_bias_score", 64)),
    (lambda: bias_score(desc(**E), bias(), ldc=10, w=0.3), -2, "aed_bias_score: ldc = 10 < V = 11"),
    (lambda: bias_score(desc(**E), bias(), ctc_rows=-1, w=0.3), -2, "aed_bias_score: ctc_rows = -1"),
    (lambda: bias_score(desc(**E), bias(), ldl=10, alpha=NAN), -2, "aed_bias_score: ldl = 10 < V = 11"),
    (lambda: bias_score(desc(**E), bias(), alpha=NAN), -2, "aed_bias_score: alpha or beta is not finite"),   # also without an LM
    (lambda: bias_score(desc(**E), bias(), use_eos=2), 0, None),                                        # no LM: use_eos is not looked at
    (lambda: bias_score(desc(**E), bias(), lm_image=PTR, lm_bytes=80, use_eos=2), -2, "aed_bias_score: use_eos = 2"),
    (lambda: bias_score(desc(**E), bias(), lm_image=PTR, lm_bytes=80, beta=INF), -2, "aed_bias_score: alpha or beta is not finite"),
    (lambda: bias_score(desc(**E), bias(), lm_image=PTR, lm_bytes=82), -2, LM_IMAGE % ("aed_bias_score", 82, LMSET_MAX)),
    (lambda: bias_score(desc(**E), bias(), lm_image=PTR, lm_bytes=76), -2, LM_IMAGE % ("aed_bias_score", 76, LMSET_MAX)),
    (lambda: bias_prune(desc(max_frames=0, **E), bias(image=None, image_bytes=0)), 0, None),            # prune does not read the image
    (lambda: bias_prune(desc(**E), None), -2, "aed_bias_prune: null bias record"),
    (lambda: bias_prune(desc(**E), bias(), lscratch=PTR), -2, LM_BLOB % "aed_bias_prune"),
    (lambda: bias_prune(desc(pre_beam=2, **E), None), -2, PRE_BEAM % ("aed_ngram", 2)),
    (lambda: bias_result(desc(max_frames=0, **E), bias(image=None, image_bytes=0)), 0, None),
    (lambda: bias_result(desc(**E), None), -2, "aed_bias_result: null bias record"),
    (lambda: bias_result(None, bias()), -2, "aed_bias: null descriptor"),
]


@pytest.mark.parametrize("i", range(len(EMPTY_ROWS)))
def test_empty_batch(i):
    call, rc, msg = EMPTY_ROWS[i]
    assert call() == rc
    if msg is not None:
        assert _lib.last_error() == msg


# ------------------------------------------------------------------ 3. the resets, refused before they read a header back
def ngram_reset(d, lstate=None, lstate_bytes=0, lm_image=PTR, lm_bytes=80):
    return _lib.load().m3_aed_ngram_reset(ref(d), lstate, lstate_bytes, lm_image, lm_bytes, None)


def ngram_reset_set(d, lstate=None, lstate_bytes=0, lm_image=PTR, lm_bytes=80):
    return _lib.load().m3_aed_ngram_reset_set(ref(d), lstate, lstate_bytes, lm_image, lm_bytes, PTR, None)


def bias_reset(d, b):
    return _lib.load().m3_aed_bias_reset(ref(d), ref(b), None)


RESET_ROWS = []
for name, fn, top in (("aed_ngram_reset", ngram_reset, LM_MAX), ("aed_ngram_reset_set", ngram_reset_set, LMSET_MAX)):
    RESET_ROWS += [
        (lambda fn=fn: fn(None), "aed_ngram: null descriptor"),
        (lambda fn=fn: fn(desc(pre_beam=2)), PRE_BEAM % ("aed_ngram", 2)),
        (lambda fn=fn: fn(desc(beam=1, V=1, pre_beam=1)), "aed_ngram: V = 1, a token and eos need two different ids"),
        (lambda fn=fn: fn(desc(), PTR, 767), "%s: LM state 767 bytes < required 768" % name),
        (lambda fn=fn: fn(desc(), ODD, 768), "%s: the LM state must be 16-byte aligned device memory" % name),
        (lambda fn=fn: fn(desc(), None, 768), "%s: the LM state must be 16-byte aligned device memory" % name),
        (lambda fn=fn: fn(desc(), PTR, 768, lm_bytes=82), LM_IMAGE % (name, 82, top)),
        (lambda fn=fn: fn(desc(**E), lm_bytes=76), LM_IMAGE % (name, 76, top)),
        (lambda fn=fn, top=top: fn(desc(**E), lm_bytes=top + 4), LM_IMAGE % (name, top + 4, top)),
    ]
RESET_ROWS += [
    (lambda: bias_reset(None, bias()), "aed_bias: null descriptor"),
    (lambda: bias_reset(desc(pre_beam=65), bias()), PRE_BEAM % ("aed_ngram", 65)),
    (lambda: bias_reset(desc(), None), "aed_bias_reset: null bias record"),
    (lambda: bias_reset(desc(**E), bias(image_bytes=12)), CTX_IMAGE % ("aed_bias_reset", 12)),
    (lambda: bias_reset(desc(), bias(image_bytes=CTX_MAX + 4, graph_of=PTR, state=PTR, state_bytes=512)), CTX_IMAGE % ("aed_bias_reset", CTX_MAX + 4)),
    (lambda: bias_reset(desc(), bias(graph_of=PTR, state=PTR, state_bytes=511)), "aed_bias_reset: context state 511 bytes < required 512"),
    (lambda: bias_reset(desc(), bias(graph_of=PTR, state=ODD, state_bytes=512)), "aed_bias_reset: the context state must be 16-byte aligned device memory"),
]


@pytest.mark.parametrize("i", range(len(RESET_ROWS)))
def test_resets_refused_before_the_read_back(i):
    call, msg = RESET_ROWS[i]
    assert call() == -2
    assert _lib.last_error() == msg
