"""The seams of the B = 1 fp32 MoE layer (moe_expert.hip): the self-routing expert launch whose waves route in registers
(S <= 64) and the combine that requests everything a row needs in one round trip.

Neither re-orders a floating-point operation, so every comparison here is of bits:
  * the self-routing launch + combine (m3_moe_route_expert_ffn) against the staged chain m3_moe_gate_index + m3_moe_expert_ffn
    (index launch, slab kernel, combine with mapping and b2), outputs and all five routing results, and the routing results
    against oracle/moe_index.py and the oracle's arg-max tree;
  * the combine against a CPU loop over the very slabs the expert launch left in the workspace, added in slice order;
  * the engine's logits against a child process that runs the per-work-group prologue (M3_ROUTE_WAVE=0)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from m3asr import ops
from oracle.encoder_ref import softmax_top1_tree
from oracle.moe_index import moe_index_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7          # what every routing result holds before the launch: an entry the launch leaves alone compares equal


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def _taps(S, E):
    i32 = lambda n: torch.full((n,), SENT, dtype=torch.int32, device="cuda")       # noqa: E731
    return (i32(S), torch.full((S,), float(SENT), device="cuda"), i32(S), i32(E + 1), i32(S))


# ------------------------------------------------------------------------------------------------ routing patterns
def _logits_for(winner, E, seed):
    """decisive logits: the planted winner at 6 .. 8, the others N(0, 0.8)"""
    S = len(winner)
    lg = rnd(S, E, seed=seed, scale=0.8)
    lg[torch.arange(S), torch.from_numpy(np.asarray(winner)).long()] = 6.0 + 2.0 * torch.rand(S, generator=_gen(seed + 1))
    return lg


def _patterns(S, E, seed):
    """-> list of (name, logits (S, E), row_len or None, rows_per_batch)"""
    rng = np.random.default_rng(seed)
    out = [("uniform", _logits_for(rng.integers(0, E, S), E, seed), None, 0)]
    if S in (50, 64, 65):
        out.append(("one", _logits_for(np.full(S, E - 3), E, seed + 2), None, 0))          # ranks reach S - 1, S / 16 tiles
    w = rng.integers(0, E - 1, S)
    w[w >= 2] += 1                                                                          # expert 2 stays empty
    out.append(("one-empty", _logits_for(w, E, seed + 4), None, 0))
    out.append(("ends", _logits_for(np.where(rng.integers(0, 2, S) == 1, E - 1, 0), E, seed + 6), None, 0))
    # exact ties between two maxima: (j, E/2 + j') with j' < j is where the reference's tree and 'first index' part; a whole-row tie
    lg = _logits_for(rng.integers(0, E, S), E, seed + 8)
    H = E // 2
    pairs = [(1, 0), (H - 1, 0), (H - 1, H - 2), (2, 0), (H - 1, H - 3)]
    lg[0, :] = 0.25
    for r, (j, j2) in zip(range(1, S), pairs):
        lg[r, j] = lg[r, H + j2] = 9.0
    out.append(("ties", lg, None, 0))
    # padded rows: utterances of rpb frames of which row_len[b] are real, one of them empty where there are two
    rpb = 16 if S > 16 else max(S, 1)
    B = -(-S // rpb)
    lens = rng.integers(1, rpb + 1, B).astype(np.int32)
    if B > 1:
        lens[1] = 0
    else:
        lens[0] = max(S - 1, 0)                        # (S = 1: the only row is padding)
    out.append(("padded", _logits_for(rng.integers(0, E, S), E, seed + 10), lens, rpb))
    out.append(("all-padded", _logits_for(rng.integers(0, E, S), E, seed + 12), np.zeros(B, dtype=np.int32), rpb))
    return out


def _oracle_taps(logits, row_len, rpb, E):
    S = logits.shape[0]
    r = np.arange(S)
    live = np.ones(S, dtype=bool) if row_len is None else (r % rpb) < row_len[r // rpb]
    gi = np.array([softmax_top1_tree(row) for row in logits.tolist()], dtype=np.int32)
    gi = np.where(live, gi, -1).astype(np.int32)
    mapping, acc = moe_index_ref(gi, E)
    nv = int(acc[E])
    pos = np.full(S, SENT, dtype=np.int32)
    pos[mapping[gi >= 0]] = np.nonzero(gi >= 0)[0]
    return gi, mapping, acc, pos, nv


class Weights:
    """expert weights of one (E, D, F), built once and shared by the cases that use them (never written)"""
    _cache = {}

    def __init__(self, E, D, Fh):
        self.w1, self.b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5).cuda(), rnd(E, Fh, seed=3, scale=0.1).cuda()
        self.w2, self.b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5).cuda(), rnd(E, D, seed=5, scale=0.1).cuda()
        self.lg, self.lb = (rnd(D, seed=10) * 0.2 + 1.0).cuda(), rnd(D, seed=11, scale=0.1).cuda()

    @classmethod
    def get(cls, E, D, Fh):
        key = (E, D, Fh)
        if key not in cls._cache:
            cls._cache[key] = cls(E, D, Fh)
        return cls._cache[key]


# ================================================================================================ self-routing vs staged
@pytest.mark.parametrize("S", [1, 15, 16, 17, 50, 63, 64, 65])
@pytest.mark.parametrize("E,Fh", [(8, 64), (8, 128), (32, 64), (32, 128)])
def test_self_routing_launch_equals_staged_chain(E, Fh, S):
    """m3_moe_route_expert_ffn (self-routing launch + combine) against m3_moe_gate_index + m3_moe_expert_ffn, torch.equal on
    the output and on gate_idx / gate_value / mapping / acc_histogram / pos; the integer results also against the oracle
    (arg-max tree + oracle/moe_index.py) and gate_idx against m3_softmax_top1.  S <= 64: every wave routes in registers;
    S = 65: the per-work-group prologue.  F = 64 / 128: one and two slabs.  Plain, and behind gate, residual and LayerNorm."""
    D = 32
    w = Weights.get(E, D, Fh)
    x = (rnd(S, D, seed=1) * 1.7 + 0.4).cuda()
    resid = rnd(S, D, seed=7).cuda()
    for name, logits, row_len, rpb in _patterns(S, E, seed=100 * S + E + Fh):
        tag = "S=%d E=%d F=%d %s" % (S, E, Fh, name)
        lg_d = logits.cuda()
        rl_d = torch.from_numpy(row_len).cuda() if row_len is not None else None
        gi, mapping, acc, pos, nv = _oracle_taps(logits, row_len, rpb, E)
        if name == "one":
            assert int(np.bincount(gi, minlength=E).max()) == S
        if name == "one-empty":
            assert 2 not in gi
        if name == "ends":
            assert set(gi.tolist()) <= {0, E - 1}
        if name == "ties" and S > 1:
            assert gi[1] != int(logits[1].argmax())            # the planted pair does separate the tree from 'first index'
        staged_taps = ops.moe_gate_index(lg_d, rl_d, rpb, taps=_taps(S, E))
        for full in (False, True):
            kw = dict(resid=resid, alpha=0.5, ln=(w.lg, w.lb, 1e-5)) if full else {}
            y, taps = ops.moe_route_expert_ffn(x, lg_d, w.w1, w.b1, w.w2, w.b2, row_len=rl_d, rows_per_batch=rpb,
                                               use_gate_value=full, taps=_taps(S, E), **kw)
            y_staged = ops.moe_expert_ffn(x, staged_taps[0], w.w1, w.b1, w.w2, w.b2,
                                          gate_value=staged_taps[1] if full else None, **kw)
            torch.cuda.synchronize()
            for tname, a, b in zip(("gate_idx", "gate_value", "mapping", "acc_histogram", "pos"), taps, staged_taps):
                assert torch.equal(a, b), "%s: %s differs from the staged chain's" % (tag, tname)
            assert not bool(torch.isnan(y).any()), tag + ": NaN in the output"
            assert torch.equal(y, y_staged), "%s full=%d: output differs from the staged chain, max |diff| %.3e" % (
                tag, full, float((y - y_staged).abs().max()))
        got = [t.cpu().numpy() for t in taps]
        assert np.array_equal(got[0], gi), tag + ": gate_idx vs the oracle's tree"
        assert np.array_equal(got[2], mapping), tag + ": mapping vs oracle/moe_index.py"
        assert np.array_equal(got[3], acc), tag + ": acc_histogram vs oracle/moe_index.py"
        assert np.array_equal(got[4], pos), tag + ": pos vs the oracle (entries from acc_histogram[E] on stay untouched)"
        assert np.all(got[1][gi < 0] == 0.0) and np.all(got[1][gi >= 0] > 0.0), tag + ": gate_value"
        _, top1 = ops.softmax_top1(lg_d)
        live = gi >= 0
        assert np.array_equal(top1.cpu().numpy()[live], gi[live]), tag + ": gate_idx vs m3_softmax_top1"


# ================================================================================================ combine
def _combine_case(S, D, n_slices, full, dropped=()):
    """run m3_moe_route_expert_ffn on F = 64 n_slices; -> (y, slabs (n_slices, S, D) as the expert launch left them, gate_idx,
    gate_value, operands).  The workspace is NaN beforehand: a dropped row's slab rows stay NaN."""
    E, Fh = 8, 64 * n_slices
    w = Weights.get(E, D, Fh)
    x = (rnd(S, D, seed=1) * 1.7 + 0.4).cuda()
    resid = rnd(S, D, seed=7).cuda()
    logits = _logits_for(np.random.default_rng(S + D + n_slices).integers(0, E, S), E, seed=S + D)
    row_len = None
    if dropped:
        row_len = np.array([0 if s in dropped else 1 for s in range(S)], dtype=np.int32)         # utterances of one frame
    need = ops.moe_route_expert_workspace_size(S, E, D, Fh)
    ws = torch.full((need // 4,), float("nan"), device="cuda")
    kw = dict(resid=resid, alpha=0.5, ln=(w.lg, w.lb, 1e-5)) if full else {}
    y, taps = ops.moe_route_expert_ffn(x, logits.cuda(), w.w1, w.b1, w.w2, w.b2, use_gate_value=full, workspace=ws, taps=_taps(S, E),
                                       row_len=torch.from_numpy(row_len).cuda() if row_len is not None else None,
                                       rows_per_batch=1 if row_len is not None else 0, **kw)
    torch.cuda.synchronize()
    slabs = ws[:n_slices * S * D].view(n_slices, S, D).cpu()
    return y.cpu(), slabs, taps[0].cpu(), taps[1].cpu(), w, resid.cpu()


@pytest.mark.parametrize("n_slices", [1, 2, 16])
@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("S", [1, 4, 5, 50])
def test_combine_sums_slabs_in_slice_order(S, D, n_slices):
    """No LayerNorm, no residual, alpha = 1, gate exactly 1.0: the combine's output is the fp32 sum of the slabs, slice 0 first,
    bit for bit (a CPU loop over the slabs the expert launch left)."""
    y, slabs, gi, _, _, _ = _combine_case(S, D, n_slices, full=False)
    assert bool((gi >= 0).all()) and not bool(torch.isnan(slabs).any())
    want = torch.zeros(S, D)
    for k in range(n_slices):
        want = want + slabs[k]
    assert torch.equal(y, want), "S=%d D=%d slices=%d: max |diff| %.3e" % (S, D, n_slices, float((y - want).abs().max()))


@pytest.mark.parametrize("n_slices", [1, 2, 16])
@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("S", [1, 4, 5, 50])
def test_combine_layernorm_residual(S, D, n_slices):
    """LN(resid + alpha * gate * sum of slabs) against the torch expression in fp64 on the slabs and the gate the launch left:
    1e-6 relative.  The absolute term is 1e-6 as well (16 u): the error of x - mean does not shrink with the result, and the
    normalised rows are O(1).  Row 0 (and the last row of S = 50) is dropped (padding): its slab rows are NaN and were never
    written, and it must come out as LN(resid) -- compared bit for bit with the combine's own LN(resid) through m3_moe_combine
    with mapping = -1, and with torch."""
    dropped = (0, S - 1) if S == 50 else (0,)
    y, slabs, gi, gv, w, resid = _combine_case(S, D, n_slices, full=True, dropped=dropped)
    for s in dropped:
        assert int(gi[s]) == -1 and bool(torch.isnan(slabs[:, s]).all())
    assert not bool(torch.isnan(y).any()), "NaN from a dropped row's slab rows reached the output"
    kept = gi >= 0
    tot = torch.zeros(S, D, dtype=torch.float64)
    for k in range(n_slices):
        tot = tot + slabs[k].double()
    tot[~kept] = 0.0
    pre = resid.double() + 0.5 * gv.double().view(S, 1) * tot
    want = F.layer_norm(pre, (D,), w.lg.cpu().double(), w.lb.cpu().double(), 1e-5)
    err = (y.double() - want).abs()
    bound = 1e-6 + 1e-6 * want.abs()
    print("combine LN S=%d D=%d slices=%d: worst err %.3e, %.3f of its bound" % (S, D, n_slices, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all()), "max err %.3e, worst %.3f of the bound" % (float(err.max()), float((err / bound).max()))
    none = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    base = ops.moe_combine(torch.zeros(1, D, device="cuda"), none, resid=resid.cuda(), alpha=0.5, ln=(w.lg, w.lb, 1e-5)).cpu()
    for s in dropped:
        assert torch.equal(y[s], base[s]), "dropped row %d is not LN(resid) bit for bit" % s


# ================================================================================================ engine
_CHILD = r"""
import sys
for p in ("", "/3m-asr-inference_amd", "/tests"):
    sys.path.insert(0, sys.argv[1] + p)
import numpy as np
from test_moe_b1_seams_gpu import _tiny_logits
np.save(sys.argv[2], _tiny_logits())
"""


def _tiny_logits():
    """EncoderConfig.tiny(num_experts=8) on one utterance of 206 frames: 50 rows per MoE layer"""
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig.tiny(num_experts=8)
    feat = torch.randn(1, 206, cfg.input_dim, generator=_gen(0))
    fl = torch.tensor([[206]], dtype=torch.int32)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=3), device="cuda:0")
    return eng(feat.cuda(), fl.cuda()).cpu().numpy()


def test_engine_logits_do_not_depend_on_the_switch(tmp_path):
    """The engine's logits (S = 50 <= 64: the self-routing launch with wave routing) against a fresh child process with
    M3_ROUTE_WAVE=0: the same bits.  The switch is read once per process, hence the child (one, with a time limit of its own)."""
    here = _tiny_logits()
    env = dict(os.environ, M3_ROUTE_WAVE="0")
    path = str(tmp_path / "off.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, "child failed:\n%s" % r.stderr[-2000:]
    off = np.load(path)
    assert here.shape == off.shape and here.shape[1] == 50 and np.isfinite(here).all()
    assert np.array_equal(here, off), "logits differ from M3_ROUTE_WAVE=0: max |diff| %.3e" % float(np.abs(here - off).max())
