"""Cases of the fp32 attention core at the far end of its range (test-side helper of tests/test_attention_long_gpu.py, written like
tests/attention_short_cases.py, which covers T' <= 80): work-group id arithmetic at large and non-power-of-two launches, long T',
and operands built so that the scores take a shape `randn` never gives (one-hot rows, stepping maxima, equal scores, a large
common offset, one wave holding everything).

Operands come from seeded CPU generators.  Launches go through tests/guarded.py (NaN around every input, a pattern around every
output) unless a case says otherwise.  References: stream_kernels_ref.attention_ref in float64 (the truth) and in float32 (the
error of the formula itself, the yardstick), packed_ref.packed_attention_ref for packed rows.

Bound (within): tol = 3e-5 below 130 keys (test_relpos_attention); from 130 keys on, and for every score regime at every T',
tol = max(3e-5, 4 e32) with e32 the largest error of the float32 CPU evaluation (test_relpos_attention_strided); a row passes when
|device - ref| <= tol + tol |ref|.  Device error, e32 and tol are printed before the assertion; ERRORS keeps the largest per tag.
"""
import math

import numpy as np
import torch

import guarded as G
import packed_ref as R
from m3asr import ops
from stream_kernels_ref import attention_ref

TOL = 3e-5
ERRORS = {}                                                      # group -> (largest device error, largest e32, largest tol)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.cuda().contiguous()


def within(tag, got, want, want32=None, rows=None, group=None):
    """print device error, e32 and tol, then assert element by element.  want32 = None: the fixed bound (below 130 keys)."""
    got, want = got.detach().cpu().double(), want.double()
    e32 = 0.0
    if want32 is not None:
        d32 = (want32.double() - want).abs()
        e32 = float((d32 if rows is None else d32[rows]).max())
    if rows is not None:
        got, want = got[rows], want[rows]
    tol = max(TOL, 4 * e32)
    err = (got - want).abs()
    worst = float(err.max()) if err.numel() else 0.0
    print("%s: device err %.3e, fp32 CPU err %.3e, tol %.3e (max |ref| %.3e)" % (tag, worst, e32, tol, float(want.abs().max()) if want.numel() else 0.0))
    g = ERRORS.get(group or tag.split("/")[0], (0.0, 0.0, 0.0))
    ERRORS[group or tag.split("/")[0]] = (max(g[0], worst), max(g[1], e32), max(g[2], tol))
    assert bool(torch.isfinite(got).all()), tag + ": a non-finite output"
    assert bool((err <= tol + tol * want.abs()).all()), "%s: device err %.3e over tol %.3e, worst excess %.3e" % (
        tag, worst, tol, float((err - tol - tol * want.abs()).max()))
    return worst, e32, tol


def operands(B, T, H, dk, seed):
    """randn operands as test_relpos_attention has them: every (b, h, query tile) its own data"""
    D = H * dk
    return (rnd(B * T, 3 * D, seed=seed + 1), rnd(T, D, seed=seed + 2), rnd(H, dk, seed=seed + 3, scale=0.3), rnd(H, dk, seed=seed + 4, scale=0.3))


def refs(qkv, p, u, v, lens, B, T, H, dk, chunk=0, left=-1, regime=False):
    """(float64 reference, float32 evaluation or None where the fixed bound applies)"""
    L = torch.as_tensor(lens, dtype=torch.int32)
    want = attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left)
    want32 = attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left, dtype=torch.float32) if (T >= 130 or regime) else None
    return want, want32


def launch_padded(tag, qkv, p, u, v, lens, B, T, H, dk, chunk=0, left=-1, guarded=True):
    """one padded launch -> the output as a dense device tensor; guards checked, every row written, empty utterances zero"""
    D = H * dk
    L = dev(torch.as_tensor(lens, dtype=torch.int32))
    if not guarded:
        return ops.relpos_attention(dev(qkv), dev(p), dev(u), dev(v), L, B, T, H, dk, chunk=chunk, left_chunks=left)
    gq, gp, go = G.strided_in(qkv, ld=3 * D + 4), G.strided_in(p, ld=D + 4), G.strided_out(B * T, D, ld=D + 4)
    ops.relpos_attention(gq.view, gp.view, dev(u), dev(v), L, B, T, H, dk, chunk=chunk, left_chunks=left, out=go.view)
    torch.cuda.synchronize()
    go.check(tag)
    assert not bool(go.untouched().any()), tag + ": a row is not written"
    got = G.dense(go.view)
    for b in range(B):
        if lens[b] == 0:
            assert not bool(got[b * T:(b + 1) * T].any()), tag + ": an empty utterance's rows are not zero"
    return got


def launch_packed(tag, qkv, p, u, v, lens, B, T, H, dk, chunk=0, left=-1, poison=True):
    """the packed form of the same batch -> (fp32 rows, bf16 rows, idx of the padded row of every packed row, row0).  poison: one more
    launch per utterance with NaN in every row it does not own (as attention_short_cases._run_packed), compared bit for bit."""
    D = H * dk
    len_out, row0, pad_of, P = R.row_plan(lens, T)
    L, row0_d = dev(torch.as_tensor(len_out)), dev(torch.as_tensor(row0))
    idx = torch.as_tensor(pad_of[:P].astype(np.int64))
    packed = qkv[idx]
    gp = G.strided_in(p, ld=D + 4)
    args = (gp.view, dev(u), dev(v), L, B, T, H, dk)
    gq, go, gb = G.strided_in(packed), G.strided_out(P, D), G.strided_out(P, D, torch.bfloat16)
    ops.relpos_attention_packed(gq.view, *args, out=go.view, row0=row0_d, chunk=chunk, left_chunks=left)
    ops.relpos_attention_packed(gq.view, *args, out=gb.view, row0=row0_d, chunk=chunk, left_chunks=left)
    torch.cuda.synchronize()
    go.check(tag)
    gb.check(tag + " out_bf16")
    assert not bool(go.untouched().any()) and not bool(gb.untouched().any()), tag + ": a live row is not written"
    got = G.dense(go.view)
    assert G.same_bits(G.dense(gb.view), got.to(torch.bfloat16)), tag + ": the bf16 output is not the rounded fp32 output"
    r0 = row0.tolist()
    for b in range(B if poison else 0):
        if r0[b + 1] == r0[b]:
            continue
        alone = torch.full_like(packed, float("nan"))
        alone[r0[b]:r0[b + 1]] = packed[r0[b]:r0[b + 1]]
        gn = G.strided_out(P, D)
        ops.relpos_attention_packed(G.strided_in(alone).view, *args, out=gn.view, row0=row0_d, chunk=chunk, left_chunks=left)
        torch.cuda.synchronize()
        gn.check(tag + " (NaN neighbours)")
        assert G.same_bits(G.dense(gn.view[r0[b]:r0[b + 1]]), got[r0[b]:r0[b + 1]]), tag + ": utterance %d read a row it does not own" % b
    return got, G.dense(gb.view), idx, row0


def padded_and_packed(tag, qkv, p, u, v, lens, B, T, H, dk, chunk=0, left=-1, regime=False, group=None, poison=True):
    """padded launch against float64; packed launch bit for bit against the padded rows and against packed_attention_ref"""
    want, want32 = refs(qkv, p, u, v, lens, B, T, H, dk, chunk, left, regime)
    got = launch_padded(tag + "/padded", qkv, p, u, v, lens, B, T, H, dk, chunk, left)
    within(tag + "/padded", got, want, want32, group=group)
    gpk, _, idx, row0 = launch_packed(tag + "/packed", qkv, p, u, v, lens, B, T, H, dk, chunk, left, poison)
    assert G.same_bits(gpk, got[idx.cuda()]), tag + ": packed rows differ from the padded call"
    want_pk = R.packed_attention_ref(qkv[idx], p, u, v, lens, row0, T, H, dk, chunk, left)
    within(tag + "/packed", gpk, want_pk, None if want32 is None else want32[idx], group=group)
    return got


# ------------------------------------------------------------------------------------------------------------ 1. id arithmetic
QT_ALL = [1, 2, 3, 5, 6, 7, 9, 11, 13, 17, 31, 33, 63, 64]
H_ALL = [1, 2, 3, 5, 6, 8, 12, 16]
# (B, H) with B H in 8 .. 24: a multiple of 8 (XCD map on) and not, H a power of two and not
_BH_CYCLE = [(1, 8), (3, 3), (2, 6), (3, 8), (5, 3), (2, 5), (1, 12), (7, 1), (2, 8), (3, 5), (4, 6), (11, 1), (1, 16), (3, 7)]


def qt_cases():
    """every QT at T' = 16 QT (full last tile) and 16 QT - 15 (one query in the last tile)"""
    cases = []
    for i, qt in enumerate(QT_ALL):
        for k, T in enumerate((16 * qt, 16 * qt - 15)):
            B, H = _BH_CYCLE[(2 * i + k) % len(_BH_CYCLE)] if qt < 31 else ((1, 8), (3, 3))[(i + k) % 2]
            cases.append(dict(id="QT%d-T%d-B%dH%d" % (qt, T, B, H), T=T, B=B, H=H))
    return cases


def h_cases():
    """every H with B H a multiple of 8 and not, 8 k + 1 and 8 k - 1 among them; T' = 81 (QT = 6) and 49 (QT = 4) in turn"""
    bs = {1: [8, 7, 9, 17], 2: [4, 5], 3: [8, 3, 5], 5: [8, 3, 5], 6: [4, 3], 8: [1, 3], 12: [2, 1, 3], 16: [1, 2]}
    cases = []
    for H in H_ALL:
        for k, B in enumerate(bs[H]):
            T = (81, 49)[k % 2]
            cases.append(dict(id="H%d-B%d-T%d" % (H, B, T), T=T, B=B, H=H))
    assert {c["B"] * c["H"] % 8 for c in cases} >= {0, 1, 7}
    return cases


def run_ids(c, dk=16):
    """ragged lengths (utterance 0 full), padded and packed"""
    B, T, H = c["B"], c["T"], c["H"]
    lens = [max(1, T - 5 * b) if b % 4 != 3 else 1 for b in range(B)]
    qkv, p, u, v = operands(B, T, H, dk, 100)
    return padded_and_packed(c["id"], qkv, p, u, v, lens, B, T, H, dk, group="ids", poison=False)


def sample_refs(qkv, p, u, v, B, T, H, dk, pairs, out):
    """float64 on a sample of (b, h): each as a B = 1, H = 1 problem cut out of the operands -> largest device error"""
    D = H * dk
    worst = 0.0
    for b, h in pairs:
        c = slice(h * dk, (h + 1) * dk)
        rows = qkv[b * T:(b + 1) * T].view(T, 3, D)[:, :, c].reshape(T, 3 * dk)
        want = attention_ref(rows, p[:, c], u[h:h + 1], v[h:h + 1], torch.tensor([T]), 1, T, 1, dk)
        worst = max(worst, within("sample", out[b * T:(b + 1) * T, c], want, group="ids-sample")[0])
    return worst


# ---------------------------------------------------------------------------------------------------------------- 2. long T'
LONG_T = [129, 192, 193, 256, 257, 500, 1024, 1025]
LONG_SHAPES = [(T, 64) for T in LONG_T] + [(129, 16), (1025, 16), (129, 128), (1025, 128)]
LONG_MASKS = [(0, -1), (16, -1), (16, 0), (16, 1), (16, 3), (64, 0)]


def long_lens(T):
    """one batch: full, a length on / above / below a 64-key trip, 17 (waves 2 and 3 without a key), and an empty utterance"""
    k = 64 * ((T - 1) // 64)
    return [T, k, k + 1, k - 1, 17, 0]


def run_long(T, dk, chunk, left, H=2):
    lens = long_lens(T)
    B = len(lens)
    qkv, p, u, v = operands(B, T, H, dk, 200)
    tag = "long-T%d-dk%d-chunk%d-left%d" % (T, dk, chunk, left)
    return padded_and_packed(tag, qkv, p, u, v, lens, B, T, H, dk, chunk, left, group="long")


# ----------------------------------------------------------------------------------------------------------- 4. score regimes
REGIMES = ["onehot", "ascending", "descending", "equal", "offset", "mixed"]


def onehot_keys(T):
    """the dominant key in turn in the first tile of wave 0, the last tile of wave 3, and a second-trip tile (T' > 64 only)"""
    t3 = max(t for t in range((T + 15) // 16) if t % 4 == 3)
    keys = [3, min(16 * t3 + 5, T - 1)]
    if T > 64:
        keys.append(min(85, T - 1))                              # tile 5: wave 1's second trip
    return keys


def key_scores(regime, n, T, generator):
    """target score of every key, [n][T] (n = the (b, h) pairs, or any set of rows that share keys)"""
    tile = torch.arange(T) // 16
    s = torch.zeros(n, T)
    if regime == "onehot":                                       # > 104 above all others: exp underflows to exactly 0 in fp32
        keys = onehot_keys(T)
        for i in range(n):
            s[i, keys[i % len(keys)]] = 120.0
    elif regime == "ascending":                                  # tile maxima step by 30: a wave's next tile is 120 above its last
        s += 30.0 * tile
    elif regime == "descending":                                 # corr = 1 throughout, every later probability tiny, then 0
        s += 30.0 * (tile.max() - tile)
    elif regime == "offset":
        s += 3000.0 + torch.randn(n, T, generator=generator)
    elif regime == "mixed":                                      # wave 2's tiles hold everything: the other three factors underflow
        s += 150.0 * (tile % 4 == 2)
    return s


def score_weight(dk):
    """(q + u)[channel 0], a power of two so that its product with a key's channel 0 is exact"""
    return 4.0 if dk == 16 else 8.0


def regime_operands(regime, B, T, H, dk, seed, bf16_rows=False):
    """finite operands whose scores ((q + u) . k + (q + v) . p) / sqrt(dk) are key_scores + a spread of about 0.5:
    (q + u)[0] = W, k[0] = score sqrt(dk) / W; the other channels of q are 0.1 randn, of k randn, p = 0.3 randn.
    equal: u = v, q = -u, so every score is exactly 0.  offset: u = v with channel 0 zero and q + u = W e_0 exactly, so a score is
    W (k[0] + p[0]) / sqrt(dk) with one rounding near 3000 -- noise added to an accumulator that large would be the test's own error.
    bf16_rows: qkv, p, u, v are bf16 values (q + u is then exact in fp32)."""
    g = torch.Generator().manual_seed(seed)
    D, W, root = H * dk, score_weight(dk), math.sqrt(dk)
    r16 = (lambda t: t.to(torch.bfloat16).float()) if bf16_rows else (lambda t: t)
    u, v = r16(torch.randn(H, dk, generator=g) * 0.3), r16(torch.randn(H, dk, generator=g) * 0.3)
    q = r16(torch.randn(B, T, H, dk, generator=g) * 0.1)
    k, vv = torch.randn(B, T, H, dk, generator=g), torch.randn(B, T, H, dk, generator=g)
    p = torch.randn(T, H, dk, generator=g) * 0.3
    s = key_scores(regime, B * H, T, g).view(B, H, T).permute(0, 2, 1)          # [B][T][H]
    if regime == "equal":
        v = u.clone()
        q = (-u).expand(B, T, H, dk).clone()
    elif regime == "offset":
        u[:, 0] = 0.0
        v = u.clone()
        q = (-u).expand(B, T, H, dk).clone()
        q[..., 0] = W
        k[..., 0] = s * (root / W)
    else:
        q[..., 0] = W - u[:, 0]
        k[..., 0] = s * (root / W)
    if bf16_rows and regime == "offset":                         # bf16 holds 3000 only to +-8: the offset in k, the spread in p
        k[..., 0] = 3008.0 * (root / W)
        p[..., 0] = torch.randn(T, H, generator=g)
    qkv = r16(torch.stack([q, k, vv], 2).reshape(B * T, 3 * D))
    return qkv, r16(p.reshape(T, D)), u, v


def regime_ok(tag, want, want32):
    """a regime whose float32 CPU evaluation is itself off by more than 1e-3 of the largest output is badly built"""
    e32, top = float((want32.double() - want).abs().max()), float(want.abs().max())
    assert e32 <= 1e-3 * top, "%s: the float32 yardstick is off by %.3e (largest |ref| %.3e): fix the inputs" % (tag, e32, top)
