"""CPU tier of the long-form path: the segmenter restatement on hand-made cases, VadConfig's refusals,
LongFormTranscriber.plan_batches on random segment lists, and the transcriber's refusal of a max_segment the positional
table cannot take.  Nothing here needs a device."""
import types

import numpy as np
import pytest

import vad_cases
import vad_ref as R
from m3asr.config import EncoderConfig, subsampled_len
from m3asr.frontend import VadConfig
from m3asr.longform import LongFormTranscriber, LongSegment


@pytest.mark.parametrize("case", vad_cases.cases(), ids=lambda c: c[0])
def test_restatement_on_hand_made_cases(case):
    _, flags, logE, n, want = case
    assert R.segments(flags, logE, n, *vad_cases.OPTS) == want


def test_restatement_log_energy_and_decide():
    x = np.full(400 + 160 * 3 + 159, 7.0)
    e, n = R.log_energy(x, T=6)
    assert n == 4 and np.all(e[:4] == np.log(R.FLT_EPSILON)) and not e[4:].any()
    assert R.log_energy(np.zeros(399))[1] == 0
    logE = np.array([0, 10, 10, 0, 0, 10, 0, 99], dtype=np.float32)
    f, thr = R.decide(logE, 7, 5.0, 0.0, 0, 0.6)
    assert thr == 5.0 and f.tolist() == [0, 1, 1, 0, 0, 1, 0, 0]
    f, thr = R.decide(logE, 7, 1.0, 0.5, 1, 0.6)                    # mean 30 / 7; windows of 2 at the edges, 3 inside
    assert abs(float(thr) - (1.0 + 15.0 / 7)) < 1e-6 and f.tolist() == [0, 1, 1, 0, 0, 0, 0, 0]


def test_vad_config_defaults_and_frames():
    c = VadConfig()
    assert (c.energy_threshold, c.energy_mean_scale, c.context, c.proportion_threshold) == (5.0, 0.5, 0, 0.6)    # Kaldi's
    assert c.segment_options() == (30, 20, 10, 3000, 500)
    assert c.frames(300) == 30 and c.frames(301) == 31 and c.frames(295.5) == 30
    assert R.options_ok(*c.segment_options())


@pytest.mark.parametrize("kw,msg", [
    (dict(context=-1), "context"), (dict(context=33), "context"),
    (dict(proportion_threshold=0.0), "proportion"), (dict(proportion_threshold=1.0), "proportion"),
    (dict(energy_mean_scale=-0.1), "energy_mean_scale"),
    (dict(min_silence=-1, pad=0), "negative"), (dict(pad=-1), "negative"),
    (dict(min_speech=6), "min_speech"),
    (dict(pad=16), "exceeds min_silence"), (dict(min_silence=19), "exceeds min_silence"),
    (dict(split_search=2994), "split_search"), (dict(max_segment=506), "split_search"), (dict(split_search=0), "split_search"),
])
def test_vad_config_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        VadConfig(**kw)
    o = dict(min_silence=30, min_speech=20, pad=10, max_segment=3000, split_search=500)
    o.update({k: v for k, v in kw.items() if k in o})
    if set(kw) <= set(o):
        assert not R.options_ok(o["min_silence"], o["min_speech"], o["pad"], o["max_segment"], o["split_search"])


def test_vad_config_edges_are_accepted():
    VadConfig(context=32, pad=15, min_silence=30, split_search=2993, min_speech=7, energy_mean_scale=0.0)
    VadConfig(pad=0, min_silence=0, max_segment=8, split_search=1)


class _Planner(LongFormTranscriber):
    """plan_batches needs the three numbers only"""

    def __init__(self, max_batch, max_batch_frames, bucket):
        self.max_batch, self.max_batch_frames, self.bucket = max_batch, max_batch_frames, bucket


@pytest.mark.parametrize("seed", range(100))
def test_plan_batches(seed):
    rng = np.random.default_rng(seed)
    max_batch, bucket = int(rng.integers(1, 9)), int(rng.choice([1, 7, 50, 100]))
    longest = int(rng.integers(7, 900))
    max_batch_frames = -(-longest // bucket) * bucket * int(rng.integers(1, 6)) + int(rng.integers(0, bucket))
    segs, t = [], 0
    for _ in range(int(rng.integers(0, 40))):
        t += int(rng.integers(0, 50))
        n = int(rng.integers(1, longest + 1))
        segs.append((t, t + n))
        t += n
    plan = _Planner(max_batch, max_batch_frames, bucket).plan_batches(segs)
    R.check_plan(segs, plan, max_batch, max_batch_frames, bucket)
    # greedy: a batch that is not the last could not have taken one segment more
    for idx, T_max in plan[:-1]:
        assert len(idx) == max_batch or (len(idx) + 1) * T_max > max_batch_frames


def test_plan_batches_refuses_what_cannot_fit():
    p = _Planner(4, 200, 100)
    with pytest.raises(ValueError, match="max_batch_frames"):
        p.plan_batches([(0, 201)])
    with pytest.raises(ValueError, match="empty"):
        p.plan_batches([(5, 5)])
    assert p.plan_batches([]) == []
    assert p.plan_batches([(0, 7), (10, 210), (300, 400)]) == [([1], 200), ([2, 0], 100)]


def test_transcriber_refuses_a_segment_the_positional_table_cannot_take():
    """the refusal comes before anything touches a device: an engine stand-in with a config is enough"""
    cfg = EncoderConfig.tiny()
    eng = types.SimpleNamespace(cfg=cfg, device="cpu")
    most = max(t for t in range(7, 4 * cfg.max_len + 16) if subsampled_len(t) < cfg.max_len)
    with pytest.raises(ValueError, match="positional table"):
        LongFormTranscriber(eng, vad=VadConfig(max_segment=most + 1), bucket=1)
    assert most % 100 >= 2                                               # so most - 1 fits, but not once it is rounded up to the bucket
    with pytest.raises(ValueError, match="positional table"):
        LongFormTranscriber(eng, vad=VadConfig(max_segment=most - 1), bucket=100)
    with pytest.raises(ValueError, match="max_batch_frames"):
        LongFormTranscriber(eng, max_batch_frames=2999)


def test_long_segment_defaults():
    assert LongSegment(0, 10, [1]).times is None
