"""WFST decoding from the command line: tools/make_lexicon_graph.py writes a graph image from a lexicon file, and
infer.py --wfst --words prints, for a synthetic checkpoint, the words (and with --timestamps their times) that CtcWfstSearch
finds in process on the same plan, which is what the host restatement finds on the same log-probabilities."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import wfst_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_lexicon_tool_and_infer_wfst(tmp_path):
    from m3asr import ops
    from m3asr.engine import Engine
    from m3asr.plan import load_plan
    from m3asr.wfst import DecodingGraph, wfst_from_logits
    d = str(tmp_path)
    _run(["tools/make_synthetic_checkpoint.py", "--out-dir", d, "--tiny", "--seed", "3"])
    plan = os.path.join(d, "enc.plan")
    _run(["builder.py", "-c", os.path.join(d, "config.yaml"), "-m", os.path.join(d, "model.pt"), "-o", plan, "--opt-shape", "2x64"])
    cfg, packed, _ = load_plan(plan)
    V = cfg.output_dim
    feat = np.random.default_rng(1).random((2, 120, 40), dtype=np.float32)
    np.save(os.path.join(d, "feat.npy"), feat)
    # a closed vocabulary: every token a one-token word w<t>, and two-token words of neighbours
    lines = ["w%d %d" % (t, t) for t in range(1, V)] + ["p%d %d %d" % (t, t, t + 1) for t in range(1, V - 1)]
    with open(os.path.join(d, "lexicon.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(d, "costs.txt"), "w") as f:
        f.write("".join("p%d 0.5\n" % t for t in range(1, V - 1)))
    graph_path, words_path = os.path.join(d, "graph.npy"), os.path.join(d, "words.txt")
    said = _run(["tools/make_lexicon_graph.py", os.path.join(d, "lexicon.txt"), "--vocab-size", str(V), "-o", graph_path,
                 "--words-out", words_path, "--word-costs", os.path.join(d, "costs.txt")])
    assert "%d words" % (2 * V - 3) in said
    printed = _run(["infer.py", "-p", plan, "-i", os.path.join(d, "feat.npy"), "--wfst", graph_path, "--words", words_path,
                    "--wfst-beam", "6", "--wfst-max-active", "64", "--timestamps"])
    shown = {int(m.group(1)): m.group(2).split() for m in re.finditer(r"^utt (\d+) wfst: cost=\S+ final=1 words=(.*)$", printed, re.M)}
    assert sorted(shown) == [0, 1], printed[-2000:]
    times = re.findall(r"^utt \d+ wfst times:\n((?:\S+ \d+\n)*)", printed, re.M)
    assert len(times) == 2 and "greedy times" not in printed

    graph = DecodingGraph.load(graph_path).to("cuda")
    names = {i + 1: line.split()[0] for i, line in enumerate(lines)}
    eng = Engine(cfg, packed, device="cuda:0")
    x = torch.from_numpy(feat).cuda()
    logits = eng(x, torch.full((1, 2), 120, dtype=torch.int32).cuda())
    T = logits.shape[1]
    got = wfst_from_logits(logits, [T, T], graph, beam=6.0, max_active=64, detail=True)
    logp = ops.log_softmax_bias(logits).cpu().numpy()
    for b in range(2):
        want = R.RefSearch(graph, 6.0, 64).advance(logp[b]).result(True)
        assert got[b]["words"] == want["words"] and got[b]["frames"] == want["frames"] and len(want["words"]) >= 1
        assert shown[b] == [names[w] for w in want["words"]]
        assert times[b].split() == [s for w, f in zip(want["words"], want["frames"]) for s in (names[w], str(40 * f))]
    # without --wfst the output has no such line
    assert "wfst" not in _run(["infer.py", "-p", plan, "-i", os.path.join(d, "feat.npy")])
