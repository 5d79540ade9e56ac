"""LM sets where sessions live: StreamPool.open(lm=j) over a StreamingCtcDecoder(lm=NgramLmSet), through an endpoint cut, against
three single-purpose pools; and infer.py with several --lm and --lm-use against the run with that LM alone."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lm_ref
from m3asr.config import EncoderConfig
from m3asr.decode import EndpointConfig, StreamingCtcDecoder
from m3asr.engine import Engine
from m3asr.serve import StreamPool
from m3asr.weights import make_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, MAXF, L_FRAMES, BEAM = 4, 16, 10, 4
LENGTH_RULE = EndpointConfig(rules=((False, 0, L_FRAMES * 40),))      # 10 frames: fires in a slot's third chunk
ALPHA, BETA, SCALES = 0.75, 0.25, (1.0, 0.5)


def _arpa(V, order, seed, bos):
    return lm_ref.random_arpa(np.random.default_rng(seed), V, order, min(V - 1, 40), 80 if order > 1 else 0, bos=bos)[1]


def test_pool_sessions_with_their_own_members_equal_single_purpose_pools():
    """three sessions of 5 chunks (one cut after the third chunk, then an open segment of two), opened with lm=1, lm=2 and
    lm=False in one pool over a set; each must equal the same session in a pool whose decoder has that LM alone (with the scaled
    weight), or none"""
    from m3asr.lm import NgramLm, NgramLmSet
    cfg = EncoderConfig(num_blocks=2, embed_blocks=2, causal=True, embed_causal=True, static_chunk_size=C, num_decoding_left_chunks=2)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=47), packed_rows=False)
    V = cfg.output_dim
    lms = [NgramLm.from_arpa(_arpa(V, 3, 5, True), None, vocab_size=V), NgramLm.from_arpa(_arpa(V, 2, 6, False), None, vocab_size=V)]
    g = torch.Generator().manual_seed(23)
    feats = [torch.rand(4 * C * 5 + 3, cfg.input_dim, generator=g) for _ in range(3)]

    def run(dec, opens):
        pool = StreamPool(dec, segment=True)
        sids = [pool.open(**kw) for kw in opens]
        for sid, f in zip(sids, feats):
            pool.push(sid, f)
        segs = [[] for _ in sids]
        for _ in range(40):
            live = pool.step()
            for i, sid in enumerate(sids):
                segs[i] += [tuple(s) for s in pool.segments(sid)]
            if not live:
                break
        return [(segs[i], pool.close(sid)) for i, sid in enumerate(sids)]

    def decoder(**kw):
        return StreamingCtcDecoder(eng.streaming(3, MAXF, independent=True), beam=BEAM, endpoint=LENGTH_RULE, **kw)

    lmset = NgramLmSet(lms, SCALES).to(eng.device)
    got = run(decoder(lm=lmset, lm_weight=ALPHA, length_bonus=BETA), [dict(lm=1), dict(lm=2), dict(lm=False)])
    want0 = run(decoder(lm=lms[0].to(eng.device), lm_weight=ALPHA * float(np.float32(SCALES[0])), length_bonus=BETA), [{}] * 3)
    want1 = run(decoder(lm=lms[1].to(eng.device), lm_weight=ALPHA * float(np.float32(SCALES[1])), length_bonus=BETA), [{}] * 3)
    plain = run(decoder(), [{}] * 3)
    assert all(len(segs) == 1 for segs, _ in want0), "every session is cut once"
    assert got[0] == want0[0] and got[1] == want1[1]
    # the session without the LM: the plain pool's prefixes and scores (a fused decoder's n-best also carries bonus and lm = 0)
    strip = lambda nbest: [tuple(h[:2]) for h in nbest]               # noqa: E731
    assert [strip(s[3]) for s in got[2][0]] == [strip(s[3]) for s in plain[2][0]] and strip(got[2][1]) == strip(plain[2][1])
    # the members matter on these sessions: the two single-purpose pools disagree
    assert want0[0] != want1[0] and want0[1] != want1[1]
    with pytest.raises(ValueError, match="above 2"):
        StreamPool(decoder(lm=lmset, lm_weight=ALPHA), segment=True).open(lm=3)


def test_infer_cli_with_two_lms_and_lm_use(tmp_path):
    """infer.py --lm a.arpa --lm b.arpa:0.5 --lm-use 1 --lm-weight 0.8 prints what --lm b.arpa --lm-weight 0.4 prints"""
    d = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "3m-asr-inference_amd"))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_checkpoint.py"), "--out-dir", d, "--tiny",
                           "--seed", "3"], env=env)
    plan = os.path.join(d, "enc.plan")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "builder.py"), "-c", os.path.join(d, "config.yaml"), "-m",
                           os.path.join(d, "model.pt"), "-o", plan, "--opt-shape", "2x64"], env=env, stdout=subprocess.DEVNULL)
    np.save(os.path.join(d, "feat.npy"), np.random.default_rng(0).random((1, 206, 40), dtype=np.float32))
    V = EncoderConfig.tiny().output_dim
    a, b = os.path.join(d, "a.arpa"), os.path.join(d, "b.arpa")
    open(a, "w").write(_arpa(V, 3, 1, True))
    open(b, "w").write(_arpa(V, 2, 2, True))

    def lines(*extra):
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "infer.py"), "-p", plan, "-i", os.path.join(d, "feat.npy"),
                                       "--beam", "4"] + list(extra), env=env, text=True)
        return [ln for ln in out.splitlines() if ln.startswith("utt ")]

    both = lines("--lm", a, "--lm", b + ":0.5", "--lm-use", "1", "--lm-weight", "0.8")
    alone = lines("--lm", b, "--lm-weight", "0.4")
    assert both == alone and any("fused" in ln and "lm=" in ln for ln in both)
    assert lines("--lm", a, "--lm", b + ":0.5", "--lm-weight", "0.8") != both          # --lm-use 0: the other member


def test_transcribe_stream_cli_with_two_lms_and_lm_use(tmp_path):
    """tools/transcribe_stream.py --synthetic 2 --lm a.arpa --lm b.arpa:0.5 --lm-use 1 --lm-weight 0.8 prints the segments of
    --lm b.arpa --lm-weight 0.4"""
    V = EncoderConfig().output_dim
    a, b = str(tmp_path / "a.arpa"), str(tmp_path / "b.arpa")
    open(a, "w").write(_arpa(V, 3, 1, True))
    open(b, "w").write(_arpa(V, 2, 2, True))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "3m-asr-inference_amd")]))

    def lines(*extra):
        r = subprocess.run([sys.executable, "tools/transcribe_stream.py", "--synthetic", "2", "--beam", "4", "--rule", "0,0,1000"] +
                           list(extra), cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return [ln for ln in r.stdout.splitlines() if " ms rule " in ln]

    both = lines("--lm", a, "--lm", b + ":0.5", "--lm-use", "1", "--lm-weight", "0.8")
    assert len(both) >= 2 and both == lines("--lm", b, "--lm-weight", "0.4")
