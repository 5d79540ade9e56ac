"""The fp32 attention core (relpos_attention_kernel, relpos_attention_dual_kernel) at short T', through ops.relpos_attention,
ops.relpos_attention_packed and ops.relpos_attention_pair.  Cases and launches: tests/attention_short_cases.py.

  T' in {1, 15, 16, 17, 33, 48, 49, 50, 63, 64, 65, 80} (64 | 65: every wave has one key tile | wave 0 takes the loop's second
  trip), dk in {16, 32, 64, 128}, (B, H) in {(1, 8), (2, 4), (1, 2), (3, 1)} (XCD map on and off); lengths full and ragged (17:
  waves 2 and 3 without a key; 1; 0: zero rows); chunk 16 with left -1 / 0 / 1 at T' = 33 and 50 (rows whose first key tiles are
  invisible); a row0 plan with unowned rows, those rows poisoned with NaN, the bf16 copy; the four dual instantiations with
  T' = 50 next to T' = 33.  All operands are row-strided views inside guard buffers (tests/guarded.py).

Checks per case:
  (a) the float64 reference within 3e-5 + 3e-5 |ref|, the bound test_relpos_attention_strided derives for T' < 130;
  (b) bit for bit what the build recorded in tests/golden/attention_short.json computed (tools/record_attention_golden.py; the
      build recorded is the one before the merge, the first-tile form and the set-up of attention.hip changed, so this
      is "no floating-point operation changed its operands or its order").  The outputs of three small cases are kept raw in
      attention_short_raw.npz: when those differ the message names the first differing element.  The digests hold for the
      recorded toolchain: another compiler may order the same source differently, so a different toolchain FAILS with that
      message rather than skipping;
  (c) dual = the two single launches, packed = padded on owned rows, guards untouched (inside run_case).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_short_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = A.all_cases()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "attention_short.json")) as f:
        rec = json.load(f)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_device_isa
    here = check_device_isa.hipcc_version()
    assert here == rec["toolchain"], ("tests/golden/attention_short.json was recorded with %s, this build's compiler is %s: the recorded bits "
                                      "hold for the recorded toolchain only -- record again on the parent build (tools/record_attention_golden.py)"
                                      % (rec["toolchain"], here))
    return rec["digests"], np.load(os.path.join(GOLDEN, "attention_short_raw.npz"))


def test_every_case_is_recorded(recorded):
    digests, raw = recorded
    assert len(digests) >= len(CASES) and len(raw.files) >= 3
    assert len({c["id"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_attention_short(case, recorded):
    digests, raw = recorded
    for r in A.run_case(case):
        if r.want is not None:
            err = (r.got.double() - r.want).abs()
            print("%s max abs err %.3e (max |ref| %.3e)" % (r.name, float(err.max()), float(r.want.abs().max())))
            assert bool((err <= A.TOL + A.TOL * r.want.abs()).all()), "%s: max abs err %.3e against fp64" % (r.name, float(err.max()))
        assert r.name in digests, r.name + " has no recorded digest"
        if r.name in raw.files:
            want = torch.from_numpy(raw[r.name])
            diff = (r.got.view(torch.int32) != want.view(torch.int32)).nonzero()
            assert diff.numel() == 0, "%s: %d element(s) differ from the recorded output, first at %s: %r recorded, %r now" % (
                r.name, diff.shape[0], diff[0].tolist(), float(want[tuple(diff[0])]), float(r.got[tuple(diff[0])]))
        assert A.digest(r.got) == digests[r.name], r.name + ": the output's bits differ from the recorded build's"
