"""LM sets on the host: the set image (m3asr.lm.NgramLmSet, include/m3asr.h "LM set"), what m3_ctc_lm_validate makes of a set,
m3_ctc_ngram_set_member, the Python-side refusals, and the SELECTIVITY of the cases the GPU tests use (tests/lm_set_cases.py):
no GPU is needed for any of it."""
import math

import numpy as np
import pytest

import lm_set_cases as cases
from m3asr import _lib, ops
from m3asr.lm import NgramLm, NgramLmSet, SET_MAGIC, lm_flags, load_lms

HDR, ENTRY = 8, 4


def _f32bits(v):
    return int(np.float32(v).view(np.int32))


# ------------------------------------------------------------------------------------------------ 1. the image
def test_pack_layout_and_round_trip(tmp_path):
    lms = cases.members()
    s = NgramLmSet(lms, cases.SCALES)
    img = s.image
    assert img.dtype == np.int32 and img[:8].tolist() == [0x534C334D, 1, cases.V, 3, img.size, 0, 0, 0] and SET_MAGIC == 0x534C334D
    end = HDR + 3 * ENTRY
    for j, m in enumerate(lms):
        off, n, scale, zero = (int(v) for v in img[HDR + ENTRY * j:HDR + ENTRY * (j + 1)])
        assert off % 4 == 0 and off >= end and n == m.image.size and scale == _f32bits(cases.SCALES[j]) and zero == 0
        assert img[off:off + n].tobytes() == m.image.tobytes()                 # the member, byte for byte
        end = off + n
    assert end == img.size
    assert len(s) == 3 and s[1] is lms[1] and s.vocab_size == cases.V and s.validate() is s
    path = str(tmp_path / "set.npy")
    s.save(path)
    t = NgramLmSet.load(path)
    assert np.array_equal(t.image, img) and len(t) == 3 and t.scales == list(cases.SCALES) and t.vocab_size == cases.V
    for a, b in zip(t.lms, lms):
        assert np.array_equal(a.image, b.image) and (a.start, a.order, a.n_states) == (b.start, b.order, b.n_states)
        assert a.score([3, 4, 5], eos=True) == b.score([3, 4, 5], eos=True)
    with pytest.raises(ValueError, match="not an LM set"):
        lms[0].save(path)
        NgramLmSet.load(path)
    # default scales: 1.0
    assert NgramLmSet(lms[:2]).scales == [1.0, 1.0]


def test_members_differ_in_start_states_and_tables():
    lms = cases.members()
    assert [m.order for m in lms] == [1, 2, 3] and [m.has_bos for m in lms] == [True, False, True]
    assert len({m.n_states for m in lms}) == 3 and len({m.start for m in lms}) >= 2 and lms[2].start != 0
    assert len({m.image.size for m in lms}) == 3


# ------------------------------------------------------------------------------------------------ 2. validate
def _entry(img, j, field):
    return HDR + ENTRY * j + field


def _mutations(s):
    img, lms = s.image, s.lms
    off = [int(img[_entry(img, j, 0)]) for j in range(3)]
    out = []

    def mut(name, needle, fn):
        bad = img.copy()
        fn(bad)
        out.append((name, needle, bad))

    mut("G = 0", "G = 0", lambda a: a.__setitem__(3, 0))
    mut("G = 65", "G = 65", lambda a: a.__setitem__(3, 65))
    mut("unaligned offset", "not a multiple of 4", lambda a: a.__setitem__(_entry(a, 1, 0), off[1] + 1))
    mut("overlap", "overlaps", lambda a: a.__setitem__(_entry(a, 1, 0), off[0]))
    mut("entry past the end", "past the end", lambda a: a.__setitem__(_entry(a, 2, 1), int(a[_entry(a, 2, 1)]) + 4))
    mut("member for another V", "built for V = %d" % (cases.V + 1), lambda a: a.__setitem__(off[1] + 2, cases.V + 1))
    mut("scale NaN", "scale", lambda a: a.__setitem__(_entry(a, 0, 2), _f32bits(float("nan"))))
    mut("scale 0", "scale", lambda a: a.__setitem__(_entry(a, 2, 2), _f32bits(0.0)))
    # a truncated member: the last member loses its last four words, the set and its directory say so consistently
    cut = img[:-4].copy()
    cut[4] = cut.size
    cut[_entry(cut, 2, 1)] -= 4
    out.append(("truncated member", "member 2", cut))
    return out


def test_validate_refuses_each_malformed_set_by_name():
    s = cases.lm_set()
    ops.ctc_lm_validate(s.image, cases.V)
    muts = _mutations(s)
    assert len(muts) == 9
    for name, needle, bad in muts:
        with pytest.raises(_lib.M3Error) as e:
            ops.ctc_lm_validate(bad, cases.V)
        assert needle in str(e.value), (name, str(e.value))
    with pytest.raises(_lib.M3Error, match="asked for V = %d" % (cases.V + 1)):
        ops.ctc_lm_validate(s.image, cases.V + 1)
    with pytest.raises(_lib.M3Error, match="says .* words"):
        ops.ctc_lm_validate(s.image[:-1], cases.V)


def test_a_single_image_still_validates():
    for m in cases.members():
        ops.ctc_lm_validate(m.image, cases.V)
        with pytest.raises(_lib.M3Error, match="asked for V"):
            ops.ctc_lm_validate(m.image, cases.V + 1)


# ------------------------------------------------------------------------------------------------ 3. set_member + host routine
def test_set_member_then_host_routine_equals_the_routine_on_the_original():
    s = cases.lm_set()
    x = cases.ctc_logits()
    for j, m in enumerate(s.lms):
        member, scale = ops.ctc_lm_set_member(s.image, j)
        assert member.tobytes() == m.image.tobytes() and scale == cases.SCALES[j]
        assert np.shares_memory(member, s.image)
        for b in range(cases.B):
            assert cases.host_search(x[b], member, cases.weight(j)) == cases.host_search(x[b], m.image, cases.weight(j))
    for j in (-1, 3):
        with pytest.raises(_lib.M3Error, match="outside"):
            ops.ctc_lm_set_member(s.image, j)
    with pytest.raises(_lib.M3Error, match="not an LM set"):
        ops.ctc_lm_set_member(s.lms[0].image, 0)
    bad = s.image.copy()
    bad[3] = 0
    with pytest.raises(_lib.M3Error, match="G = 0"):
        ops.ctc_lm_set_member(bad, 0)


# ------------------------------------------------------------------------------------------------ 4. Python refusals
def test_python_refusals():
    lms = cases.members()
    with pytest.raises(ValueError, match="no members"):
        NgramLmSet([])
    with pytest.raises(ValueError, match="65 members"):
        NgramLmSet([lms[0]] * 65)
    NgramLmSet([lms[0]] * 64)
    other = NgramLm.from_arpa(cases.arpa_texts()[0], None, vocab_size=cases.V + 1)
    with pytest.raises(ValueError, match="vocabulary"):
        NgramLmSet([lms[0], other])
    for bad in (float("nan"), float("inf"), 0.0, -1.0, 1e-60, 1e60):
        with pytest.raises(ValueError, match="scale"):
            NgramLmSet(lms, [1.0, bad, 1.0])
    with pytest.raises(ValueError, match="scales"):
        NgramLmSet(lms, [1.0])
    s = NgramLmSet(lms, cases.SCALES)
    # lm_on: ints for a set, flags for a single LM; an id above the set is refused
    assert lm_flags(s, None, 3, "t") == [1, 1, 1]
    assert lm_flags(s, [True, False, 3, 0, 1], 5, "t") == [1, 0, 3, 0, 1]
    assert lm_flags(s, [-1], 1, "t") == [-1]
    with pytest.raises(ValueError, match="above 3"):
        lm_flags(s, [4], 1, "t")
    for bad in (1.5, "x", None):
        with pytest.raises(ValueError, match="whole number"):
            lm_flags(s, [bad], 1, "t")
    assert lm_flags(s, [2.0], 1, "t") == [2]
    with pytest.raises(_lib.M3Error, match="above 3"):
        lm_flags(s, [4], 1, "t", _lib.M3Error)
    with pytest.raises(ValueError, match="2 entries"):
        lm_flags(s, [1, 2], 3, "t")
    assert lm_flags(lms[0], [True, 0, 7], 3, "t") == [1, 0, 1]                 # a single LM: today's meaning


def test_command_line_lm_options(tmp_path):
    paths = []
    for j, text in enumerate(cases.arpa_texts()):
        p = tmp_path / ("m%d.arpa" % j)
        p.write_text(text)
        paths.append(str(p))
    lm, on = load_lms([paths[0]], None, cases.V)
    assert isinstance(lm, NgramLm) and on is None                              # one --lm: exactly as before
    lm, on = load_lms([paths[0], paths[1] + ":0.5"], None, cases.V, 1)
    assert isinstance(lm, NgramLmSet) and on == 2 and lm.scales == [1.0, 0.5]
    lm, on = load_lms([paths[2] + ":2"], None, cases.V)
    assert isinstance(lm, NgramLmSet) and on == 1 and lm.scales == [2.0]
    lm, on = load_lms([paths[0]], None, cases.V, 0)
    assert isinstance(lm, NgramLmSet) and on == 1
    with pytest.raises(ValueError, match="use = 2"):
        load_lms(paths[:2], None, cases.V, 2)


# ------------------------------------------------------------------------------------------------ 5. selectivity
def _selective(x, lms, what):
    """the host routine under the three members (each with its scaled weight): pairwise different hyp_lm of the best
    hypothesis, at least two different best hypotheses"""
    got = [cases.host_search(x, m.image, cases.weight(j)) for j, m in enumerate(lms)]
    best_lm = [g[0][3] for g in got]
    assert len(set(best_lm)) == 3, (what, best_lm)
    for a in range(3):
        for b in range(a + 1, 3):
            assert [h[3] for h in got[a]] != [h[3] for h in got[b]], (what, a, b)
    assert len({g[0][0] for g in got}) >= 2, (what, [g[0][0] for g in got])


def test_the_gpu_cases_are_selective():
    lms = cases.members()
    x = cases.ctc_logits()
    for b in range(cases.B):
        _selective(x[b], lms, "ctc utterance %d" % b)
        for t0 in (7, 9, 10):                                       # the frames a restarted slot sees in the streaming cases
            _selective(x[b, t0:], lms, "ctc utterance %d from frame %d" % (b, t0))


def test_scaled_weight_is_one_double_product():
    assert cases.weight(0) == cases.ALPHA and cases.weight(1) == cases.ALPHA * 0.5 and cases.weight(2) == cases.ALPHA * 2.0
    assert all(math.isfinite(cases.weight(j)) for j in range(3))
