"""The routing launches of the B = 1 fp32 MoE layer, called directly (m3_moe_gate_index, m3_moe_route, m3_moe_route_expert_ffn)
against the oracle's arg-max tree, the numpy index contract and fp64 arithmetic, on guarded operands (tests/guarded.py: NaN
around every input, a bit pattern around every output that must survive; the expert workspace holds signalling NaNs, so a slab
row that is read without having been written shows in the result).

Routing never hinges on rounding: where the device computes the logits (m3_moe_route) every row keeps an fp64 top-2 margin
well above the logit tolerance (rows that do not are redrawn on the CPU, none is excluded); exact ties are planted only where
the device sees the very same floats as the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded as G
from m3asr import ops, _lib
from m3asr._lib import M3Error
from oracle.encoder_ref import softmax_top1_tree
from oracle.moe_index import moe_index_ref

U = 2.0 ** -24          # unit roundoff of fp32
GATE_RTOL, GATE_ATOL = 1e-5, 1e-7      # the bound test_softmax_top1 holds for the gate value on given logits


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ oracle side
def _tie_pairs(E):
    """(j, E/2 + j') with j' < j: both hold the row maximum; the tree keeps the LOWER SLOT of the first stage, E/2 + j', where
    'first index' would say j.  One pair per later tree stage (the stride at which slots j and j' meet), and the two ends."""
    H = E // 2
    pairs = [(1, 0), (H - 1, 0), (H - 1, H - 2)]
    pairs += [(j, j - s) for s in (2, 4, 8, 16) for j in (s, H - 1) if j < H and j - s >= 0]
    return sorted(set(p for p in pairs if 0 <= p[1] < p[0] < H))


def _plant_ties(logits, rows=None):
    """row rows[0]: a whole-row tie; the following rows: one pair each (as many as fit).  Returns the planted rows."""
    S, E = logits.shape
    rows = list(range(S)) if rows is None else rows
    planted = []
    if rows:
        logits[rows[0], :] = 0.25
        planted.append(rows[0])
    for r, (j, j2) in zip(rows[1:], _tie_pairs(E)):
        logits[r, j] = logits[r, E // 2 + j2] = float(np.ceil(float(logits[r].max()))) + 1.0      # (an integer: exact in any sum below)
        planted.append(r)
    return planted


def _live_rows(S, row_len, rpb):
    if row_len is None:
        return np.ones(S, dtype=bool)
    r = np.arange(S)
    return (r % rpb) < np.asarray(row_len)[r // rpb]


def _route_ref(logits, live):
    """logits (S, E) fp32 as the device sees them -> gate_idx (tree rule), gate_value (fp64), mapping, acc, pos, kept rows"""
    S, E = logits.shape
    l64 = logits.double()
    gi = np.array([softmax_top1_tree(row) for row in logits.tolist()], dtype=np.int32)
    assert np.array_equal(l64.numpy()[np.arange(S), gi], l64.max(-1).values.numpy())          # the tree's pick is a maximum
    gv = (1.0 / torch.exp(l64 - l64.max(-1, keepdim=True).values).sum(-1)).numpy()
    gi = np.where(live, gi, -1).astype(np.int32)
    gv = np.where(live, gv, 0.0)
    mapping, acc = moe_index_ref(gi, E)
    nv = int(acc[E])
    pos = np.full(S, -1, dtype=np.int32)
    pos[mapping[gi >= 0]] = np.nonzero(gi >= 0)[0]
    return gi, gv, mapping, acc, pos, nv


class Taps:
    """guarded output buffers of the five routing results"""

    def __init__(self, S, E):
        self.S, self.E = S, E
        self.gi, self.gv = G.flat_out((S,), torch.int32), G.flat_out((S,), torch.float32)
        self.mp, self.acc, self.pos = G.flat_out((S,), torch.int32), G.flat_out((E + 1,), torch.int32), G.flat_out((S,), torch.int32)

    def views(self):
        return (self.gi.view, self.gv.view, self.mp.view, self.acc.view, self.pos.view)

    def check(self, want, tag, gate_rtol=GATE_RTOL):
        """integers exact, pos untouched from acc[E] on, gate value within gate_rtol / GATE_ATOL; returns the worst gate error
        in units of its bound"""
        gi, gv, mapping, acc, pos, nv = want
        for name, g_ in (("gate_idx", self.gi), ("gate_value", self.gv), ("mapping", self.mp), ("acc_histogram", self.acc), ("pos", self.pos)):
            g_.check("%s: %s" % (tag, name))
        assert np.array_equal(self.gi.view.cpu().numpy(), gi), tag + ": gate_idx"
        assert np.array_equal(self.mp.view.cpu().numpy(), mapping), tag + ": mapping"
        assert np.array_equal(self.acc.view.cpu().numpy(), acc), tag + ": acc_histogram"
        assert np.array_equal(self.pos.view.cpu().numpy()[:nv], pos[:nv]), tag + ": pos"
        assert bool(self.pos.untouched()[nv:].all()), tag + ": pos written at or beyond acc_histogram[E]"
        got = self.gv.view.cpu().double().numpy()
        assert not bool(self.gv.untouched().any()), tag + ": gate_value not written everywhere"
        assert np.all(got[gi < 0] == 0.0), tag + ": gate_value of a dropped row"
        err, bound = np.abs(got - gv), GATE_ATOL + gate_rtol * np.abs(gv)
        assert np.all(err <= bound), "%s: gate_value err %.3e" % (tag, float(err.max()))
        return float((err / bound).max())


def _row_lens(mode, S, rng):
    """-> (row_len or None, rows_per_batch): ragged utterances incl. a length-0 one where there are two, or all dead"""
    if mode == "null":
        return None, 0
    rpb = 64 if mode == "ragged64" else 50
    B = -(-S // rpb)
    if mode == "dead":
        return np.zeros(B, dtype=np.int32), rpb
    lens = rng.integers(1, rpb + 1, B).astype(np.int32)
    lens[0] = rpb                      # (the planted ties live in the first rows)
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = rpb - 1
    return lens, rpb


# ================================================================================================ m3_moe_gate_index
@pytest.mark.parametrize("S", [1, 64, 65, 256, 1025, 2100])
@pytest.mark.parametrize("E", [8, 16, 32, 64])
def test_moe_gate_index(E, S):
    """SoftmaxTopK + ScatterMapping in one launch on given logits: gate_idx by the reference's arg-max tree (planted: a whole-row
    tie and pairs (j, E/2 + j') where the tree and 'first index' disagree), mapping / acc_histogram / pos bit-exact against the
    numpy contract, pos untouched from acc_histogram[E] on, gate_value within test_softmax_top1's 1e-5 / 1e-7 of fp64.
    row_len: NULL, ragged utterances of 50 and of 64 frames (one of length 0, the last one cut short by S), all dead."""
    rng = np.random.default_rng(S * 7 + E)
    logits = rnd(S, E, seed=S + E, scale=4.0)
    planted = _plant_ties(logits)
    assert len(planted) == min(S, 1 + len(_tie_pairs(E)))
    lg = G.flat_in(logits)
    worst = 0.0
    for mode in ("null", "ragged50", "ragged64", "dead"):
        row_len, rpb = _row_lens(mode, S, rng)
        live = _live_rows(S, row_len, rpb)
        want = _route_ref(logits, live)
        if mode in ("null", "ragged50", "ragged64"):
            assert live[planted].all()
            first_index = logits[planted].argmax(-1).numpy()
            assert S < 2 or (want[0][planted][1:] != first_index[1:]).all()           # the planted pairs do separate the two rules
        rl = G.flat_in(torch.from_numpy(row_len), int_guard=0) if row_len is not None else None
        t = Taps(S, E)
        ops.moe_gate_index(lg.view, rl.view if rl else None, rpb, taps=t.views())
        torch.cuda.synchronize()
        worst = max(worst, t.check(want, "gate_index E=%d S=%d %s" % (E, S, mode)))
    print("gate_index E=%d S=%d: worst gate_value err %.3f of its bound (%g rel + %g abs)" % (E, S, worst, GATE_RTOL, GATE_ATOL))


@pytest.mark.parametrize("E,S", [(4, 8), (12, 8), (16, 0)])
def test_moe_gate_index_rejects(E, S):
    lib = _lib.load()
    logits = torch.zeros(64, 64, device="cuda")
    t = Taps(64, 64)
    with pytest.raises(M3Error):
        _lib.check(lib.m3_moe_gate_index(_ptr(logits), None, 0, S, E, *[_ptr(v) for v in t.views()], _stream()), "m3_moe_gate_index")
    torch.cuda.synchronize()
    assert all(bool(g_.untouched().all()) for g_ in (t.gi, t.gv, t.mp, t.acc, t.pos))


# ================================================================================================ m3_moe_route
ROUTE_S = [1, 15, 16, 17, 50, 80, 255, 256]
MARGIN = 1e-3


def _folded_logits64(x, wx, wsum, bias, eall, eps):
    """fp64 of the folded algebra on the operands the device gets: (x . wx^T - mean * wsum) * rstd + bias + eall"""
    x64 = x.double()
    mean = x64.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mean) ** 2).mean(-1, keepdim=True) + eps)
    y = (x64 @ wx.double().t() - mean * wsum.double().view(1, -1)) * rstd + eall.double()
    return y + bias.double().view(1, -1) if bias is not None else y


def _top2_margin(l64):
    top = l64.topk(2, dim=-1).values
    return top[:, 0] - top[:, 1]


@pytest.mark.parametrize("D", [16, 80, 512])
@pytest.mark.parametrize("E", [16, 32, 64])
def test_moe_route(E, D):
    """moe_route_kernel at every S of its work split (S = 80: 5 tiles x 3 K-parts, one wave idle; 15 / 16 / 17 / 255 / 256: tile
    edges; 1), rows of mean 0 and of mean 10 (the folded LayerNorm's cancellation), bias present (strided x with ldx > D and
    eall with ld_e > E, NaN around the rows) and NULL (dense operands), ragged row_len on the S >= 50 cases.
    Reference: fp64 of the folded algebra on the very fp32 operands.  The logits are compared through gate_value:
    d(gate_value) / gate_value <= 2 max|d logit|, and the suite's law for the folded one-pass statistics
    (test_linear_folded_layernorm) is |d logit| <= tol (1 + |logit|) with tol = max(3e-5, 6e-5 |mean| / std); so the bound is
    rtol = 1e-5 + 2 tol (1 + max|logit|), atol 1e-7.  Every row's fp64 top-2 margin is >= max(1e-3, 4 tol (1 + max|logit|)):
    rows below it are redrawn from the next seed, and none may be left."""
    Smax, eps = 256, 1e-5
    wx = rnd(E, D, seed=11 + E + D, scale=D ** -0.5)
    wsum = wx.double().sum(1).float()
    bias = rnd(E, seed=12 + E, scale=0.5)
    wx_d, wsum_d, bias_d = G.flat_in(wx), G.flat_in(wsum), G.flat_in(bias)
    rng = np.random.default_rng(E + D)
    for mean in (0.0, 10.0):
        tol = max(3e-5, 6e-5 * abs(mean) / 1.0)
        x = rnd(Smax, D, seed=21 + E + D) + mean
        eall = rnd(Smax, E, seed=22 + E + D, scale=1.5)
        for use_bias in (True, False):
            b = bias if use_bias else None
            # ---- margins: redraw the rows whose two best logits are too close for a comparison of integers
            for k in range(1, 40):
                l64 = _folded_logits64(x, wx, wsum, b, eall, eps)
                dl = tol * (1.0 + float(l64.abs().max()))
                bad = (_top2_margin(l64) < max(MARGIN, 4 * dl)).nonzero().view(-1).tolist()
                if not bad:
                    break
                for r in bad:
                    x[r] = torch.randn(D, generator=_gen(1000 * k + r)) + mean
                    eall[r] = torch.randn(E, generator=_gen(2000 * k + r)) * 1.5
            assert not bad, "rows %s keep a top-2 margin below the bar" % bad
            gate_rtol = GATE_RTOL + 2 * dl
            worst = 0.0
            for S in ROUTE_S:
                if use_bias:
                    xg, eg = G.strided_in(x[:S].contiguous()), G.strided_in(eall[:S].contiguous(), ld=E + 8)
                    assert xg.ld > D and xg.ld % 4 == 0 and eg.ld > E
                else:
                    xg, eg = G.flat_in(x[:S].contiguous()), G.flat_in(eall[:S].contiguous())
                row_len, rpb = _row_lens("ragged50" if S >= 50 and not use_bias else "null", S, rng)
                live = _live_rows(S, row_len, rpb)
                want = _route_ref(l64[:S].float(), live)                     # (margins >> fp32 rounding of the fp64 logits)
                gv64 = 1.0 / torch.exp(l64[:S] - l64[:S].max(-1, keepdim=True).values).sum(-1)
                want = (want[0], np.where(live, gv64.numpy(), 0.0)) + want[2:]
                rl = G.flat_in(torch.from_numpy(row_len), int_guard=0) if row_len is not None else None
                t = Taps(S, E)
                ops.moe_route(xg.view, wx_d.view, wsum_d.view, bias_d.view if use_bias else None, eg.view, eps,
                              rl.view if rl else None, rpb, taps=t.views())
                torch.cuda.synchronize()
                worst = max(worst, t.check(want, "route E=%d D=%d S=%d mean=%g bias=%d" % (E, D, S, mean, use_bias), gate_rtol))
            print("route E=%d D=%d mean=%g bias=%d: worst gate_value err %.3f of its bound (rtol %.2e: logit tolerance %.2e)"
                  % (E, D, mean, use_bias, worst, gate_rtol, dl))


@pytest.mark.parametrize("S", [1, 17, 50, 256])
@pytest.mark.parametrize("E", [16, 32, 64])
def test_moe_route_exact_ties(E, S):
    """wx = 0, wsum = 0: the logits are eall + bias exactly (quarter-integer bias, ties planted in the sum), so the 16-lane
    arg-max of phase B must follow the reference's tree on a whole-row tie and on pairs (j, E/2 + j') at rows of the first
    and of the last wave; also all rows dead."""
    D = 16
    x = rnd(S, D, seed=S) * 3.0 + 1.0
    wx, wsum = torch.zeros(E, D), torch.zeros(E)
    for use_bias in (False, True):
        bias = (torch.randint(-4, 5, (E,), generator=_gen(E)).float() / 4.0) if use_bias else torch.zeros(E)
        total = rnd(S, E, seed=E + S)                     # what the device must see
        last = list(range(S - 1, max(S - 1 - len(_tie_pairs(E)), S // 2), -1))
        planted = _plant_ties(total) + (_plant_ties(total, last) if S > 2 * (1 + len(_tie_pairs(E))) else [])
        eall = total - bias.view(1, -1)
        logits = eall + bias.view(1, -1)                  # fp32, the device's own sum
        assert bool(((logits[planted] == logits[planted].max(-1, keepdim=True).values).sum(-1) >= 2).all())   # the ties survive the sum
        for mode in ("null", "dead"):
            row_len, rpb = _row_lens(mode, S, None)
            live = _live_rows(S, row_len, rpb)
            want = _route_ref(logits, live)
            if mode == "null" and S > 1:
                assert (want[0][planted[1:2]] != logits[planted[1:2]].argmax(-1).numpy()).all()
            rl = G.flat_in(torch.from_numpy(row_len), int_guard=0) if row_len is not None else None
            t = Taps(S, E)
            ops.moe_route(G.strided_in(x).view, wx.cuda(), wsum.cuda(), bias.cuda() if use_bias else None,
                          G.strided_in(eall, ld=E + 4).view, 1e-5, rl.view if rl else None, rpb, taps=t.views())
            torch.cuda.synchronize()
            t.check(want, "route ties E=%d S=%d bias=%d %s" % (E, S, use_bias, mode))


@pytest.mark.parametrize("S,E,D,ldx", [(257, 16, 16, 16), (50, 8, 16, 16), (50, 16, 24, 24), (50, 16, 16, 18)])
def test_moe_route_rejects(S, E, D, ldx):
    lib = _lib.load()
    x, wx, ws, ea = (torch.zeros(300, 64, device="cuda") for _ in range(4))
    t = Taps(300, 64)
    with pytest.raises(M3Error):
        _lib.check(lib.m3_moe_route(_ptr(x), ldx, D, _ptr(wx), _ptr(ws), None, _ptr(ea), 64, 1e-5, None, 0, S, E,
                                    *[_ptr(v) for v in t.views()], _stream()), "m3_moe_route")
    torch.cuda.synchronize()
    assert all(bool(g_.untouched().all()) for g_ in (t.gi, t.gv, t.mp, t.acc, t.pos))


# ================================================================================================ m3_moe_route_expert_ffn
def _winners(routing, S, E, rng):
    """expert per row, planted through the logits; -> (winner[S], row_len mode)"""
    if routing in ("uniform", "ties", "dead", "ragged"):
        return rng.integers(0, E, S), {"dead": "dead", "ragged": "ragged50"}.get(routing, "null")
    if routing == "one":
        return np.full(S, E - 3), "null"
    assert routing == "skewed"
    # chosen experts get exactly 16, 17, 32 and 33 rows (tile edges of the 16-row tile, and of the 32-row tile of S > 64), one
    # gets 1 row, one the rest (more than a tile), the others none; 50 rows only hold the first two edges
    counts = [16, 17, 32, 33, 1] if S >= 99 else [16, 17, 1]
    experts = rng.permutation(E)[:len(counts) + 1]
    w = np.concatenate([np.full(c, e) for c, e in zip(counts, experts)] + [np.full(S - sum(counts), experts[-1])])
    return rng.permutation(w), "null"


def _route_logits(routing, S, E, rng, seed):
    w, len_mode = _winners(routing, S, E, rng)
    logits = rnd(S, E, seed=seed, scale=0.8)
    # the winner at 6 .. 8, the others N(0, 0.8): decisive (6 is 7.5 sigma), gate values spread over about 0.8 .. 0.98
    logits[torch.arange(S), torch.from_numpy(w).long()] = 6.0 + 2.0 * torch.rand(S, generator=_gen(seed + 1))
    if routing == "ties":
        _plant_ties(logits)
    return logits, len_mode


OPT_KEYS = ("w2_sliced", "norm", "ln", "gate", "resid", "alpha")
O_OFF = dict(w2_sliced=0, norm=0, ln=0, gate=0, resid=0, alpha=1.0)
O_ON = dict(w2_sliced=1, norm=1, ln=1, gate=1, resid=1, alpha=0.5)
O_ENG = dict(w2_sliced=1, norm=0, ln=1, gate=1, resid=1, alpha=0.5)       # what the engine's staged route runs
O_MIX = dict(w2_sliced=0, norm=1, ln=0, gate=1, resid=1, alpha=1.0)
O_RES = dict(w2_sliced=1, norm=0, ln=0, gate=0, resid=1, alpha=0.5)

# every option on and off in a balanced and in a one-expert routing (O_OFF / O_ON in both); every S, E, F, D of the list;
# (S <= 64: 16-row tiles, else 32-row tiles)
FFN_CASES = [
    (1, 8, 16, 64, "uniform", O_OFF), (1, 32, 512, 256, "one", O_ON),
    (16, 16, 512, 64, "one", O_OFF),            # exactly one full tile
    (17, 32, 16, 256, "one", O_ON),             # one row into the second tile
    (17, 8, 16, 64, "ties", O_OFF),
    (64, 64, 512, 256, "uniform", O_ON), (64, 8, 512, 64, "one", O_OFF),      # 64 rows on one expert: 4 tiles in one work-group
    (64, 16, 16, 64, "ragged", O_MIX),
    (65, 8, 512, 256, "uniform", O_OFF), (65, 64, 16, 64, "one", O_ON),
    (255, 32, 512, 64, "skewed", O_ENG), (255, 16, 16, 256, "ragged", O_MIX),
    (256, 8, 512, 64, "one", O_ON),             # 256 rows on one expert: 8 tiles in one work-group
    (256, 8, 512, 64, "one", O_OFF),
    (256, 64, 512, 256, "skewed", O_OFF), (256, 32, 16, 64, "uniform", O_RES), (256, 32, 512, 64, "ties", O_ENG),
    (256, 16, 512, 256, "dead", O_ON), (50, 32, 512, 256, "dead", O_RES), (50, 32, 16, 64, "dead", O_OFF),
    (50, 8, 512, 1024, "uniform", O_ENG),
    # D > 512: the 16-row tile passes 64 KB of LDS from D = 960 on
    (50, 8, 1024, 64, "uniform", O_ON), (64, 8, 2048, 64, "one", O_OFF), (16, 16, 2048, 64, "uniform", O_ON),
    (1, 8, 1024, 128, "one", O_MIX), (65, 8, 1024, 64, "uniform", O_ON), (65, 8, 1024, 64, "one", O_OFF),
]


def _ffn_id(c):
    return "S%d-E%d-D%d-F%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "".join(str(int(c[5][k] != O_OFF[k])) for k in OPT_KEYS))


class FfnProblem:
    """operands (CPU + guarded device copies) and the fp64 reference of one m3_moe_route_expert_ffn case"""

    def __init__(self, S, E, D, Fh, routing, seed=0):
        self.S, self.E, self.D, self.F = S, E, D, Fh
        rng = np.random.default_rng(S * 1000 + E + D + Fh + seed)
        self.logits, len_mode = _route_logits(routing, S, E, rng, seed=31 + S + E)
        self.row_len, self.rpb = _row_lens(len_mode, S, rng)
        self.live = _live_rows(S, self.row_len, self.rpb)
        self.route = _route_ref(self.logits, self.live)
        self.x = rnd(S, D, seed=1) * 1.7 + 0.4
        self.w1, self.b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
        self.w2, self.b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
        self.resid = rnd(S, D, seed=7)
        self.ng, self.nb = rnd(D, seed=8) * 0.2 + 1.0, rnd(D, seed=9, scale=0.1)
        self.lg, self.lb = rnd(D, seed=10) * 0.2 + 1.0, rnd(D, seed=11, scale=0.1)
        self.eps = 1e-5
        self.dev = {k: G.flat_in(getattr(self, k)) for k in ("logits", "w1", "b1", "w2", "b2", "resid", "ng", "nb", "lg", "lb")}
        self.dev["x"] = G.strided_in(self.x)
        self.dev["row_len"] = G.flat_in(torch.from_numpy(self.row_len), int_guard=0) if self.row_len is not None else None
        self._ffn64 = {}

    def ffn64(self, norm):
        """fp64 SiLU(xn W1^T + b1) W2^T + b2 of every kept row, touched experts only (0 for dropped rows); shared by the options"""
        if norm not in self._ffn64:
            x64 = self.x.double()
            if norm:
                x64 = F.layer_norm(x64, (self.D,), self.ng.double(), self.nb.double(), self.eps)
            y = torch.zeros(self.S, self.D, dtype=torch.float64)
            gi = self.route[0]
            for e in np.unique(gi[gi >= 0]):
                rows = torch.from_numpy(np.nonzero(gi == e)[0])
                h = x64[rows] @ self.w1[e].double().t() + self.b1[e].double()
                y[rows] = (h * torch.sigmoid(h)) @ self.w2[e].double().t() + self.b2[e].double()
            self._ffn64[norm] = y
        return self._ffn64[norm]

    def want64(self, o):
        gi, gv = self.route[0], self.route[1]
        gate = torch.from_numpy(gv if o["gate"] else (gi >= 0).astype(np.float64)).view(-1, 1)
        y = o["alpha"] * gate * self.ffn64(o["norm"])
        if o["resid"]:
            y = y + self.resid.double()
        return F.layer_norm(y, (self.D,), self.lg.double(), self.lb.double(), self.eps) if o["ln"] else y

    def run(self, o, tag):
        """-> (y guarded, taps); guards and routing results checked"""
        S, E, D, Fh, d = self.S, self.E, self.D, self.F, self.dev
        need = ops.moe_route_expert_workspace_size(S, E, D, Fh)
        assert need >= (Fh // 64) * S * D * 4
        ws = G.flat_out((need // 4,), torch.float32)          # the fill pattern is a signalling NaN
        yg, t = G.flat_out((S, D)), Taps(S, E)
        ops.moe_route_expert_ffn(d["x"].view, d["logits"].view, d["w1"].view, d["b1"].view, d["w2"].view, d["b2"].view,
                                 row_len=d["row_len"].view if d["row_len"] else None, rows_per_batch=self.rpb,
                                 w2_sliced=bool(o["w2_sliced"]), norm=(d["ng"].view, d["nb"].view, self.eps) if o["norm"] else None,
                                 use_gate_value=bool(o["gate"]), resid=d["resid"].view if o["resid"] else None, alpha=o["alpha"],
                                 ln=(d["lg"].view, d["lb"].view, self.eps) if o["ln"] else None, workspace=ws.view, out=yg.view,
                                 taps=t.views())
        torch.cuda.synchronize()
        ws.check(tag + ": workspace")
        yg.check(tag + ": y")
        assert not bool(yg.untouched().any()), tag + ": y not written everywhere"
        worst_gate = t.check(self.route, tag)
        return yg, t, worst_gate


def _ffn_tol(ln):
    """the suite's bounds for this arithmetic (test_fmoe_expert: 3e-5 / 3e-5 on the FFN output, 5e-5 / 5e-5 behind gate, residual
    and the final LayerNorm; resid + alpha * gate * y without the LayerNorm adds three roundings, 4u (|term| + |resid|) << 3e-5,
    and keeps the first).  D = 1024 and 2048 need no more: fp32 MFMA accumulation errs like sqrt(n) u, not n u, and the weights
    are scaled by D^-1/2; the wide cases are held to the same figures."""
    return 5e-5 if ln else 3e-5


def _dead_rows_exact(p, o, y, tag):
    """a dropped row is resid (or 0), or the combine's own LayerNorm of it, bit for bit"""
    dead = torch.from_numpy(p.route[0] < 0)
    if not bool(dead.any()):
        return
    S, D = p.S, p.D
    base = p.dev["resid"].view if o["resid"] else torch.zeros(S, D, device="cuda")
    if o["ln"]:
        none = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        base = ops.moe_combine(torch.zeros(1, D, device="cuda"), none, resid=p.dev["resid"].view if o["resid"] else None,
                               alpha=o["alpha"], ln=(p.dev["lg"].view, p.dev["lb"].view, p.eps))
    assert G.same_bits(y[dead.cuda()], base[dead.cuda()]), tag + ": a dropped row is not resid / LN(resid) exactly"


@pytest.mark.parametrize("case", FFN_CASES, ids=_ffn_id)
def test_moe_route_expert_ffn(case):
    """The self-routing expert launch + its combine against fp64  LN(resid + alpha * gate * (SiLU(xn W1^T + b1) W2^T + b2)),
    touched experts only; the five routing results exact / within the gate bound; dropped rows exact.  Tolerance: _ffn_tol.
    D > 512 with S <= 64 needs more than 64 KB of dynamic LDS for the 16-row tile (136 KB at D = 2048), in instantiations that
    are not opted into large LDS: on gfx950 the launch succeeds without the opt-in and computes the right rows."""
    S, E, D, Fh, routing, o = case
    p = FfnProblem(S, E, D, Fh, routing)
    tag = "route_ffn " + _ffn_id(case)
    gi = p.route[0]
    if routing == "one":
        assert int(np.bincount(gi[gi >= 0], minlength=E).max()) == S
    if routing == "skewed":
        assert {16, 17, 32, 33, 1} <= set(np.bincount(gi, minlength=E).tolist()) and int((np.bincount(gi, minlength=E) == 0).sum()) >= 2
    if routing == "dead":
        assert (gi < 0).all()
    if routing == "ragged":
        assert (gi < 0).any() and (gi >= 0).any()
    yg, t, worst_gate = p.run(o, tag)
    want = p.want64(o)
    got = yg.view.cpu().double()
    tol = _ffn_tol(o["ln"])
    err, bound = (got - want).abs(), tol + tol * want.abs()
    print("%s: worst err %.3e (%.3f of its bound, tol %.2e); gate_value %.3f of its bound" % (
        tag, float(err.max()), float((err / bound).max()), tol, worst_gate))
    assert bool((err <= bound).all()), "%s: max err %.3e, worst excess %.3e" % (tag, float(err.max()), float((err - bound).max()))
    _dead_rows_exact(p, o, yg.view, tag)


@pytest.mark.parametrize("S,E,D,Fh", [(257, 8, 16, 64), (50, 12, 16, 64), (50, 8, 24, 64), (50, 8, 16, 96), (65, 8, 2048, 64)])
def test_moe_route_expert_ffn_rejects(S, E, D, Fh):
    """Shapes the operator does not take come back as an error before any launch; (S = 65, D = 2048) would need a 272 KB tile."""
    lib = _lib.load()
    big = torch.zeros(2 * 1024 * 1024, device="cuda")
    y, ws = G.flat_out((S, D)), G.flat_out((max(Fh // 64, 1) * S * D,), torch.float32)
    t = Taps(S, E)
    with pytest.raises(M3Error):
        _lib.check(lib.m3_moe_route_expert_ffn(_ptr(big), D, _ptr(big), None, 0, _ptr(big), _ptr(big), _ptr(big), 0, _ptr(big), S, E, D, Fh,
                                               None, None, 0.0, 1, None, 1.0, None, None, 0.0, *[_ptr(v) for v in t.views()],
                                               _ptr(y.view), _ptr(ws.view), ws.view.numel() * 4, _stream()), "m3_moe_route_expert_ffn")
    torch.cuda.synchronize()
    assert bool(y.untouched().all()) and bool(ws.untouched().all()) and all(bool(g_.untouched().all()) for g_ in (t.gi, t.gv, t.mp, t.acc))


# ================================================================================================ the claim of moe_expert.hip
@pytest.mark.parametrize("routing", ["uniform", "one", "skewed", "ragged", "dead", "ties"])
@pytest.mark.parametrize("S,E,D,Fh", [(50, 32, 512, 256), (256, 8, 512, 64)])
def test_self_routing_equals_staged_bit_for_bit(S, E, D, Fh, routing):
    """moe_expert.hip: the self-routing launch is 'bit-identical to launch_moe_gate_index + launch_expert_ffn_f32_slab +
    combine(mapping, b2)'.  m3_moe_expert_ffn is that staged chain (index, slab kernel, combine with mapping and b2); it gets the
    ORACLE's gate_idx and the gate_value the new entry left (checked against fp64 above it), with and without the epilogue.
    (50 rows hold only the 16- and 17-row experts of the skewed routing.)  The fp64 bound binds as well."""
    p = FfnProblem(S, E, D, Fh, routing, seed=1)
    gi_d = torch.from_numpy(p.route[0]).cuda()
    for o in (O_OFF, dict(O_ENG, w2_sliced=0), O_ENG):
        tag = "claim S=%d E=%d %s %s" % (S, E, routing, "".join(str(int(o[k] != O_OFF[k])) for k in OPT_KEYS))
        yg, t, _ = p.run(o, tag)
        d = p.dev
        staged = ops.moe_expert_ffn(p.x.cuda(), gi_d, d["w1"].view, d["b1"].view, d["w2"].view, d["b2"].view,
                                    gate_value=t.gv.view if o["gate"] else None, resid=d["resid"].view if o["resid"] else None,
                                    alpha=o["alpha"], ln=(d["lg"].view, d["lb"].view, p.eps) if o["ln"] else None)
        torch.cuda.synchronize()
        diff = (yg.view - staged).abs()
        print("%s: self-routing vs staged max |diff| %.3e (%d of %d elements differ)" % (
            tag, float(diff.max()), int((G._bits(yg.view.contiguous()) != G._bits(staged)).sum()), staged.numel()))
        assert G.same_bits(yg.view, staged), tag + ": not bit-identical, max diff %.3e" % float(diff.max())
        want = p.want64(o)
        tol = _ffn_tol(o["ln"])
        err = (yg.view.cpu().double() - want).abs()
        assert bool((err <= tol + tol * want.abs()).all()), "%s: max err %.3e" % (tag, float(err.max()))


# ================================================================================================ m3_moe_expert_ffn, D > 512
@pytest.mark.parametrize("S,E,D,Fh", [(50, 8, 1024, 128), (50, 8, 2048, 64), (200, 8, 1024, 128)])
def test_fmoe_expert_wide_rows(S, E, D, Fh):
    """The plain slab kernel (given gate_idx) beyond D = 512, which test_fmoe_expert stops at: 16-row tiles of more than 64 KB
    (S <= 64) and the 32-row tile of S = 200.  fp64 reference; test_fmoe_expert's own tolerances (3e-5 / 3e-5 plain, 5e-5 / 5e-5 behind the
    epilogue): the wider rows need no more."""
    assert _lib.load().m3_moe_expert_ffn_kernel(0, 0, S, E, D, Fh, None, None) == b"expert_ffn_f32_kernel"
    rng = np.random.default_rng(S + D)
    g = rng.integers(-1, E, S).astype(np.int32)
    x = rnd(S, D, seed=1)
    w1, b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
    w2, b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
    gate, res = torch.rand(S, generator=_gen(6)), rnd(S, D, seed=7)
    ga, be = rnd(D, seed=8) * 0.2 + 1.0, rnd(D, seed=9, scale=0.1)
    y64 = torch.zeros(S, D, dtype=torch.float64)
    for e in np.unique(g[g >= 0]):
        rows = torch.from_numpy(np.nonzero(g == e)[0])
        h = x.double()[rows] @ w1[e].double().t() + b1[e].double()
        y64[rows] = (h * torch.sigmoid(h)) @ w2[e].double().t() + b2[e].double()
    dv = [G.flat_in(t_) for t_ in (x, w1, b1, w2, b2)]
    g_d = G.flat_in(torch.from_numpy(g), int_guard=-1)
    for ln in (False, True):
        out = G.flat_out((S, D))
        kw = dict(gate_value=gate.cuda(), resid=res.cuda(), alpha=0.5, ln=(ga.cuda(), be.cuda(), 1e-5)) if ln else {}
        ops.moe_expert_ffn(dv[0].view, g_d.view, *[t_.view for t_ in dv[1:]], out=out.view, **kw)
        torch.cuda.synchronize()
        out.check("fmoe wide D=%d S=%d" % (D, S))
        want = y64
        if ln:
            want = F.layer_norm(res.double() + 0.5 * (gate.double() * torch.from_numpy(g >= 0)).view(S, 1) * y64, (D,), ga.double(), be.double(), 1e-5)
        tol = _ffn_tol(ln)
        err = (out.view.cpu().double() - want).abs()
        print("fmoe wide S=%d D=%d F=%d epilogue=%d: worst err %.3e (%.3f of its bound, tol %.2e)" % (
            S, D, Fh, ln, float(err.max()), float((err / (tol + tol * want.abs())).max()), tol))
        assert bool((err <= tol + tol * want.abs()).all()), "max err %.3e" % float(err.max())
        if not ln:
            assert bool((out.view.cpu()[torch.from_numpy(g < 0)] == 0).all())
