"""Records what the loaded library computes for the cases of tests/attention_short_cases.py: a sha256 per output in
tests/golden/attention_short.json and the raw outputs of three small cases in tests/golden/attention_short_raw.npz.
tests/test_attention_short_gpu.py then asserts that a later build computes the same bits.

Run once on the GPU, against the build whose results are to be kept (M3ASR_LIB selects a library other than the in-tree one):
    python tools/record_attention_golden.py [OUT_DIR]        (default OUT_DIR: tests/golden)
Every case's own checks (guards, fp64 reference, packed = padded, dual = single) run while recording; a case that fails them is
not recorded and the tool exits non-zero."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3m-asr-inference_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import numpy as np
import torch

import attention_short_cases as A
import check_device_isa

RAW_IDS = ["plain-T1-dk16-B1H2", "plain-T17-dk16-B1H2", "chunk16-left0-T33-dk16-B3H1"]

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
os.makedirs(out_dir, exist_ok=True)
digests, raw, worst = {}, {}, 0.0
for c in A.all_cases():
    for r in A.run_case(c):
        if r.want is not None:
            err = (r.got.double() - r.want).abs()
            worst = max(worst, float(err.max()))
            assert bool((err <= A.TOL + A.TOL * r.want.abs()).all()), "%s: max abs err %.3e" % (r.name, float(err.max()))
        digests[r.name] = A.digest(r.got)
        if c["id"] in RAW_IDS:
            raw[r.name] = r.got.numpy()
with open(os.path.join(out_dir, "attention_short.json"), "w") as f:
    json.dump({"toolchain": check_device_isa.hipcc_version(), "torch": torch.__version__, "device": torch.cuda.get_device_name(0),
               "digests": digests}, f, indent=0, sort_keys=True)
    f.write("\n")
np.savez(os.path.join(out_dir, "attention_short_raw.npz"), **raw)
print("recorded %d outputs of %d cases (%d raw), largest |error| against fp64 %.3e" % (len(digests), len(A.all_cases()), len(raw), worst))
