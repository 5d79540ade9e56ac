"""CPU: what bench.py --dump-outputs writes -- the array as fp32 .npy, or above the size limit a fixed, seeded sample of its
rows with their row numbers (the same rows from run to run).  Runs in a child process: importing bench.py sets a HIP
runtime variable for the whole process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
out = sys.argv[2]
x = np.arange(2 * 5 * 7, dtype=np.float64).reshape(2, 5, 7)
print(bench.dump_outputs(out + "/whole", "logits", x))
print(bench.dump_outputs(out + "/s1", "logits", x, limit=4 * (7 * 4 + 8)))
print(bench.dump_outputs(out + "/s2", "logits", x, limit=4 * (7 * 4 + 8)))
"""


def test_dump_outputs_whole_and_sampled(tmp_path):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    x = np.arange(2 * 5 * 7, dtype=np.float64).reshape(2, 5, 7)
    assert sorted(os.listdir(tmp_path / "whole")) == ["logits.npy"]
    whole = np.load(tmp_path / "whole" / "logits.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, x.astype(np.float32))
    got = []
    for d in ("s1", "s2"):
        assert sorted(os.listdir(tmp_path / d)) == ["logits_sample.npy", "logits_sample_rows.npy"]
        rows = np.load(tmp_path / d / "logits_sample_rows.npy")
        sample = np.load(tmp_path / d / "logits_sample.npy")
        assert rows.dtype == np.float64 and sample.dtype == np.float32 and sample.shape == (4, 7)
        assert len(np.unique(rows)) == 4 and np.all(np.diff(rows) > 0) and rows.min() >= 0 and rows.max() < 10
        assert np.array_equal(sample, x.reshape(-1, 7)[rows.astype(np.int64)].astype(np.float32))
        assert sample.nbytes + rows.nbytes <= 4 * (7 * 4 + 8)
        got.append(rows)
    assert np.array_equal(got[0], got[1])
