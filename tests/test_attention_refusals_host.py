"""The two refusals of check_relpos_attention (csrc/attention.hip) that guard the fp32 core's 32-bit arithmetic, answered on the
host before any launch (operands are placeholders that are never read; written like tests/test_packed_forms_host.py):

  span   a lane's operand address is a wave-uniform base plus a 32-bit BYTE offset (att_ld), so the rows of one utterance, T' times
         the largest of ldq / ldp / ldo, must stay below 2^30 elements.  Refused at 2^30 exactly and at 2^30 + ld, for each of the
         three strides, through every entry: padded, _chunk, _packed, _pair (each problem in turn) and the streaming entry's T ldo.
  ids    a work-group id is divided by QT = cdiv(T', 16) and by H with round-up reciprocals (att_div), exact while
         n_wg max(QT, H) < 2^32 with n_wg = QT H B.  The largest B admitted and the smallest refused follow from that inequality
         (wg_bounds below), not from asking the library.

Return code (-2, M3_REQUIRE) and the full m3_last_error() text are pinned.  The accepting side of both bounds -- a span of
2^30 - 4096 elements, launches of up to 66560 work-groups -- runs on the GPU in tests/test_attention_long_gpu.py."""
import ctypes as C

import pytest

from m3asr import _lib

_HOST = (C.c_char * 4096)()
P = (C.addressof(_HOST) + 15) // 16 * 16
N = None
LIMIT = 1 << 30

SPAN_MSG = "attention: the rows of one utterance span %d elements (T' times the largest row stride; limit 2^30)"
WG_MSG = "attention: %d work-groups are more than the kernel's id arithmetic holds"
STREAM_MSG = "attention (stream): a chunk's rows span %d elements (limit 2^30)"
PAIR_MSG = ("attention pair: head widths %d / %d (64 or 128 each) or row strides ldq %d / %d, ldp %d / %d (multiples of 4) are not a "
            "paired instantiation")


def _desc(B=1, T=1024, H=1, dk=16, ldq=None, ldp=None, ldo=None, chunk=0, left=-1):
    D = H * dk
    d = _lib.AttentionDesc()
    d.qkv, d.ldq, d.p, d.ldp, d.pos_u, d.pos_v, d.len, d.out, d.ldo = P, ldq or 3 * D, P, ldp or D, P, P, P, P, ldo or D
    d.B, d.T, d.H, d.dk, d.scale, d.chunk, d.left_chunks = B, T, H, dk, dk ** -0.5, chunk, left
    return d


def _padded(d):
    return _lib.load().m3_relpos_attention(d.qkv, d.ldq, d.p, d.ldp, d.pos_u, d.pos_v, d.len, d.B, d.T, d.H, d.dk, d.scale, d.out, d.ldo, N)


def _chunk(d):
    return _lib.load().m3_relpos_attention_chunk(d.qkv, d.ldq, d.p, d.ldp, d.pos_u, d.pos_v, d.len, d.B, d.T, d.H, d.dk, d.scale, 16, 1,
                                                 d.out, d.ldo, N)


def _packed(d):
    return _lib.load().m3_relpos_attention_packed(C.byref(d), P, 0, N)


ENTRIES = {"padded": _padded, "chunk": _chunk, "packed": _packed}
# T' ld = 2^30 exactly, and one row more: 2^30 + ld
SPANS = {"2^30": (1024, 1 << 20), "2^30+ld": (1025, 1 << 20)}


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("which", ["ldq", "ldp", "ldo"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_span_refused(entry, which, span):
    T, ld = SPANS[span]
    assert T * ld in (LIMIT, LIMIT + ld)
    rc = ENTRIES[entry](_desc(T=T, **{which: ld}))
    assert rc == -2 and _lib.last_error() == SPAN_MSG % (T * ld), (rc, _lib.last_error())


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("which", ["ldq", "ldp", "ldo"])
@pytest.mark.parametrize("problem", [0, 1])
def test_span_refused_in_a_pair(problem, which, span):
    """the paired launch asks the same check as a question (say = false) and answers with its own sentence"""
    T, ld = SPANS[span]
    good, bad = _desc(B=2, T=33, H=2, dk=128), _desc(T=T, dk=64, **{which: ld})
    pair = (bad, good) if problem == 0 else (good, bad)
    rc = _lib.load().m3_relpos_attention_pair(C.byref(pair[0]), C.byref(pair[1]), N)
    want = PAIR_MSG % (pair[0].dk, pair[1].dk, pair[0].ldq, pair[1].ldq, pair[0].ldp, pair[1].ldp)
    assert rc == -2 and _lib.last_error() == want, (rc, _lib.last_error())


def _stream(C_, ldo, H=1, dk=16):
    D = H * dk
    return _lib.load().m3_relpos_attention_stream(P, 3 * D, P, C_, P, D, C_, P, P, P, P, 1, C_, H, dk, dk ** -0.5, -1, -1, P, ldo, N)


@pytest.mark.parametrize("C_,ldo", [(16, 1 << 26), (17, 1 << 26), (1024, 1 << 20)], ids=["2^30", "2^30+ld", "2^30,C=1024"])
def test_stream_span_refused(C_, ldo):
    assert C_ * ldo in (LIMIT, LIMIT + ldo)
    rc = _stream(C_, ldo)
    assert rc == -2 and _lib.last_error() == STREAM_MSG % (C_ * ldo), (rc, _lib.last_error())


def wg_bounds(T, H):
    """(largest B admitted, smallest B refused) from  n_wg max(QT, H) < 2^32,  n_wg = QT H B:  B <= (2^32 - 1) div (QT H max(QT, H))"""
    QT = -(-T // 16)
    largest = ((1 << 32) - 1) // (QT * H * max(QT, H))
    assert QT * H * largest * max(QT, H) < (1 << 32) <= QT * H * (largest + 1) * max(QT, H)
    return largest, largest + 1


INT_MAX = (1 << 31) - 1


@pytest.mark.parametrize("entry", ENTRIES)
def test_work_group_bound_long_utterances(entry):
    """T' = 1024, H = 8: QT = 64, n_wg = 512 B, 512 B 64 < 2^32  <=>  B < 2^17.  The smallest refused B gets the work-group sentence.
    The largest admitted B is given a span of 2^30 so that no launch follows: the span is checked after the ids, so hearing the
    span sentence means the id check let B pass."""
    admit, refuse = wg_bounds(1024, 8)
    assert (admit, refuse) == (131071, 131072)
    rc = ENTRIES[entry](_desc(B=refuse, T=1024, H=8))
    assert rc == -2 and _lib.last_error() == WG_MSG % (64 * 8 * refuse), (rc, _lib.last_error())
    rc = ENTRIES[entry](_desc(B=admit, T=1024, H=8, ldq=1 << 20))
    assert rc == -2 and _lib.last_error() == SPAN_MSG % LIMIT, (rc, _lib.last_error())


@pytest.mark.parametrize("entry", ENTRIES)
def test_work_group_bound_one_tile(entry):
    """T' = 16, H = 1: QT = 1, n_wg = B and the inequality is B < 2^32: the largest B it admits is 2^32 - 1 and the smallest it
    refuses 2^32, neither of which the ABI's 32-bit B can carry.  So the work-group sentence cannot be heard at this shape; what
    can be pinned is that the largest B the ABI carries, 2^31 - 1, passes the id check (it reaches the span check behind it)."""
    admit, refuse = wg_bounds(16, 1)
    assert (admit, refuse) == ((1 << 32) - 1, 1 << 32) and refuse > INT_MAX
    rc = ENTRIES[entry](_desc(B=INT_MAX, T=16, H=1, ldq=1 << 26))
    assert rc == -2 and _lib.last_error() == SPAN_MSG % LIMIT, (rc, _lib.last_error())


@pytest.mark.parametrize("T,H", [(17, 1), (16, 3), (400, 4), (1024, 16), (8192, 8)])
def test_work_group_bound_other_shapes(T, H):
    """the same derivation where QT and H are not powers of two (the reciprocals are then inexact, which is what the bound is for)"""
    admit, refuse = wg_bounds(T, H)
    if refuse <= INT_MAX:
        QT = -(-T // 16)
        rc = _padded(_desc(B=refuse, T=T, H=H))
        assert rc == -2 and _lib.last_error() == WG_MSG % (QT * H * refuse), (rc, _lib.last_error())
    ld = -(-(-(-LIMIT // T)) // 4) * 4                    # the smallest multiple of 4 with T ld >= 2^30
    assert ld % 4 == 0 and T * ld >= LIMIT > T * (ld - 4) and ld >= 3 * H * 16
    rc = _padded(_desc(B=min(admit, INT_MAX), T=T, H=H, ldq=ld))
    assert rc == -2 and _lib.last_error() == SPAN_MSG % (T * ld), (rc, _lib.last_error())
