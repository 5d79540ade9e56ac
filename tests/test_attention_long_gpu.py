"""The fp32 attention core (csrc/attention.hip) where tests/attention_short_cases.py stops: work-group id arithmetic at large and
non-power-of-two launches, the key loop far past its second trip, operand spans up to the 2^30-element limit of the 32-bit lane
offsets, and score distributions that `randn` never produces (one-hot rows, stepping maxima, exactly equal scores, a large common
offset, one wave holding everything) -- the last also for the bf16 core, the chunk-by-chunk kernel and the attention decoder's
kernels.  Cases, operand construction and the bound are in tests/attention_long_cases.py; the refusals on the far side of the two
limits are tests/test_attention_refusals_host.py.

No bound comes from the device: float64 on the CPU is the truth, the same formula in float32 on the CPU the yardstick, and every
test prints device error, yardstick and bound before it asserts (run with -s)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_kernels_ref as kref
import attention_long_cases as A
import guarded as G
from m3asr import ops
from stream_kernels_ref import attention_ref

dev = A.dev
NAN = float("nan")


# ================================================================================================ 1. id arithmetic
@pytest.mark.parametrize("case", A.qt_cases(), ids=lambda c: c["id"])
def test_ids_query_tiles(case):
    """QT = cdiv(T', 16) over {1 .. 64}, powers of two and not, the last tile full and with one query; dk = 16"""
    A.run_ids(case)


@pytest.mark.parametrize("case", A.h_cases(), ids=lambda c: c["id"])
def test_ids_heads(case):
    """every H with the XCD map on (B H a multiple of 8) and off"""
    A.run_ids(case)


@pytest.mark.parametrize("B", [257, 256], ids=lambda b: "B%d" % b)
def test_ids_large_launch(B):
    """B = 257, H = 3, T' = 113: QT = 8, 6168 work-groups, XCD map off, H no power of two; B = 256: 768 = 8 x 96, XCD map on"""
    T, H, dk = 113, 3, 16
    assert (B * H % 8 == 0) == (B == 256)
    lens = [T if b % 3 else max(1, (37 * b) % (T + 1)) for b in range(B)]
    A.padded_and_packed("large-B%d" % B, *A.operands(B, T, H, dk, 300), lens, B, T, H, dk, group="ids", poison=False)


def test_ids_65536_work_groups():
    """B = 1040, H = 8, T' = 128, dk = 16: 66560 work-groups.  float64 on a seeded sample of 64 (b, h); every row bit for bit against
    the same problem launched as two halves of the batch (rows are independent, the halves have other ids for the same rows)."""
    B, T, H, dk = 1040, 128, 8, 16
    D = H * dk
    assert (T // 16) * H * B >= 1 << 16
    qkv, p, u, v = A.operands(B, T, H, dk, 400)
    lens = [T] * B
    out = A.launch_padded("wg65536", qkv, p, u, v, lens, B, T, H, dk, guarded=False)
    g = torch.Generator().manual_seed(5)
    pairs = [(int(b), int(h)) for b, h in zip(torch.randint(0, B, (62,), generator=g), torch.randint(0, H, (62,), generator=g))]
    pairs += [(0, 0), (B - 1, H - 1)]
    A.sample_refs(qkv, p, u, v, B, T, H, dk, pairs, out.cpu())
    half = B // 2
    for i in range(2):
        rows = slice(i * half * T, (i + 1) * half * T)
        part = A.launch_padded("wg65536 half %d" % i, qkv[rows], p, u, v, lens[:half], half, T, H, dk, guarded=False)
        assert G.same_bits(part, out[rows]), "half %d of the batch differs from the whole launch" % i
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("dk0,dk1", [(128, 64), (64, 128), (64, 64), (128, 128)], ids=lambda d: "dk%d" % d)
def test_ids_dual(dk0, dk1):
    """two problems of unequal size in one launch, both orders: n0 rounded to a multiple of 8 behind a large first problem
    (T' = 401: QT = 26, 312 work-groups; T' = 97: QT = 7, 140 work-groups), the second problem's own reciprocals"""
    probs = [dict(B=3, T=401, H=4, dk=dk0, lens=[401, 64, 385], chunk=16, left=1, seed=500),
             dict(B=5, T=97, H=4, dk=dk1, lens=[97, 17, 0, 65, 96], chunk=0, left=-1, seed=510)]
    ins, single = [], []
    for q in probs:
        B, T, H, dk = q["B"], q["T"], q["H"], q["dk"]
        D = H * dk
        qkv, p, u, v = A.operands(B, T, H, dk, q["seed"])
        want, want32 = A.refs(qkv, p, u, v, q["lens"], B, T, H, dk, q["chunk"], q["left"])
        gq, gp = G.strided_in(qkv), G.strided_in(p, ld=2 * D)
        kw = dict(qkv=gq.view, p=gp.view, pos_u=dev(u), pos_v=dev(v), lens=dev(torch.tensor(q["lens"], dtype=torch.int32)), B=B, T=T, H=H, dk=dk,
                  chunk=q["chunk"], left_chunks=q["left"])
        ins.append((kw, (B * T, D), want, want32))
        go = G.strided_out(B * T, D)
        ops.relpos_attention(out=go.view, **kw)
        torch.cuda.synchronize()
        go.check("dual single")
        single.append(G.dense(go.view))
    for order in ((0, 1), (1, 0)):
        outs = [G.strided_out(*ins[i][1]) for i in order]
        ops.relpos_attention_pair(*[dict(out=o.view, **ins[i][0]) for i, o in zip(order, outs)])
        torch.cuda.synchronize()
        for i, o in zip(order, outs):
            tag = "dual-dk%d-dk%d/order%d%d/problem%d" % (dk0, dk1, order[0], order[1], i)
            o.check(tag)
            assert not bool(o.untouched().any()), tag + ": a row is not written"
            A.within(tag, G.dense(o.view), ins[i][2], ins[i][3], group="ids-dual")
            assert G.same_bits(G.dense(o.view), single[i]), tag + ": the paired launch differs from the single launch"


# ================================================================================================ 2. long T'
@pytest.mark.parametrize("chunk,left", A.LONG_MASKS, ids=lambda x: "m%d" % x)
@pytest.mark.parametrize("T,dk", A.LONG_SHAPES, ids=lambda x: "%d" % x)
def test_long(T, dk, chunk, left):
    """one ragged batch (full, 64 k, 64 k + 1, 64 k - 1, 17 and 0 frames), padded and packed with the bf16 copy, NaN in the rows an
    utterance does not own.  Chunk 16 / left 0 at T' = 1025: most key tiles of most rows are invisible (m_new == -inf over and over,
    then left)."""
    A.run_long(T, dk, chunk, left)


# ================================================================================================ 3. the 2^30 span edge
SPAN_T, SPAN_LD = 1024, (1 << 20) - 4
LEAD_BYTES = 1 << 31


class Wide:
    """A (rows, width) operand with a row stride near 2^20 .. 2^26 elements inside one torch.empty buffer: only the operand's columns
    and 64 columns on either side are filled (NaN for an input, the guard pattern for an output).  Below the first row lie 2 GiB of
    the same allocation, filled likewise: a lane offset taken as a signed number points there, and the test then fails on a value."""

    def __init__(self, rows, width, ld, data=None):
        lead = -(-LEAD_BYTES // (4 * ld)) * ld
        self.is_output = data is None
        self.buf = torch.empty(lead + (rows - 1) * ld + 64 + width + 64, dtype=torch.float32, device="cuda")
        bits = self.buf.view(torch.int32)
        self.pattern = 0x7FA5A5A5 if self.is_output else 0x7FC00000
        bits[:lead].fill_(self.pattern)
        self.lead = bits[:lead]
        self.band = torch.as_strided(bits, (rows, 64 + width + 64), (ld, 1), lead)
        self.band.fill_(self.pattern)
        self.view = torch.as_strided(self.buf, (rows, width), (ld, 1), lead + 64)
        if data is not None:
            self.view.copy_(data)
        assert self.view.data_ptr() % 16 == 0 and self.view.stride(0) == ld
        self.width = width

    def check(self, tag):
        assert bool((self.lead == self.pattern).all()), tag + ": written below the first row"
        assert bool((self.band[:, :64] == self.pattern).all()) and bool((self.band[:, 64 + self.width:] == self.pattern).all()), tag + ": a guard column is overwritten"
        assert not bool((self.band[:, 64:64 + self.width] == self.pattern).any()), tag + ": an element is not written"


@pytest.mark.parametrize("which", ["ldq", "ldp", "ldo"])
def test_span_edge(which):
    """T' = 1024, B = H = 1, dk = 16 with one row stride of 2^20 - 4: a span of 2^30 - 4096 elements, the largest the check admits at
    this T' (the next multiple of 4 is refused); the last row's byte offset is 2^32 - 16400.  Bit for bit the dense-stride result."""
    T, dk = SPAN_T, 16
    assert T * SPAN_LD < (1 << 30) <= T * (SPAN_LD + 4)
    qkv, p, u, v = A.operands(1, T, 1, dk, 600)
    L = dev(torch.tensor([T], dtype=torch.int32))
    dense = ops.relpos_attention(dev(qkv), dev(p), dev(u), dev(v), L, 1, T, 1, dk)
    want, want32 = A.refs(qkv, p, u, v, [T], 1, T, 1, dk)
    A.within("span-edge dense", dense, want, want32, group="span")
    wide = Wide(T, {"ldq": 3 * dk, "ldp": dk, "ldo": dk}[which], SPAN_LD, {"ldq": qkv, "ldp": p, "ldo": None}[which])
    q_, p_ = (wide.view if which == "ldq" else dev(qkv)), (wide.view if which == "ldp" else dev(p))
    out = wide.view if which == "ldo" else torch.empty(T, dk, device="cuda")
    ops.relpos_attention(q_, p_, dev(u), dev(v), L, 1, T, 1, dk, out=out)
    torch.cuda.synchronize()
    if which == "ldo":
        wide.check("span-edge ldo")
    print("span-edge %s: %d elements (%d bytes to the last row)" % (which, T * SPAN_LD, (T - 1) * SPAN_LD * 4))
    assert G.same_bits(out.contiguous(), dense), "a row stride of %d gives another result: %.3e" % (SPAN_LD, float((out - dense).abs().max()))
    del wide, out, q_, p_
    torch.cuda.empty_cache()


def test_span_edge_stream():
    """the chunk-by-chunk entry: C = 16 rows of ldo = 2^26 - 4, T ldo = 2^30 - 64"""
    C_, dk, ldo = 16, 16, (1 << 26) - 4
    assert C_ * ldo < (1 << 30) <= C_ * (ldo + 4)
    qkv, p, u, v = A.operands(1, C_, 1, dk, 610)
    cl, step = dev(torch.tensor([C_], dtype=torch.int32)), torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = torch.full((1, C_, 2 * dk), NAN, device="cuda")
    dense = ops.relpos_attention_stream(dev(qkv), hist, dev(p), dev(u), dev(v), cl, step, 1, C_, 1, dk)
    want, _ = A.refs(qkv, p, u, v, [C_], 1, C_, 1, dk)
    A.within("span-edge stream dense", dense, want, group="span")
    wide = Wide(C_, dk, ldo)
    ops.relpos_attention_stream(dev(qkv), torch.full_like(hist, NAN), dev(p), dev(u), dev(v), cl, step, 1, C_, 1, dk, out=wide.view)
    torch.cuda.synchronize()
    wide.check("span-edge stream")
    assert G.same_bits(wide.view.contiguous(), dense)
    del wide
    torch.cuda.empty_cache()


# ================================================================================================ 4. score regimes
@pytest.mark.parametrize("dk", [16, 64, 128], ids=lambda d: "dk%d" % d)
@pytest.mark.parametrize("T", [50, 200], ids=lambda t: "T%d" % t)
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime_fp32(regime, T, dk):
    """padded and packed, without a mask and under chunk 16 / left 1 (rows that do not see the dominant key are ordinary rows)"""
    B, H = 3, 2
    qkv, p, u, v = A.regime_operands(regime, B, T, H, dk, 700)
    lens = [T, T, T - 9]
    for chunk, left in ((0, -1), (16, 1)):
        tag = "regime-%s-T%d-dk%d-chunk%d" % (regime, T, dk, chunk)
        want, want32 = A.refs(qkv, p, u, v, lens, B, T, H, dk, chunk, left, regime=True)
        A.regime_ok(tag, want, want32)
        got = A.padded_and_packed(tag, qkv, p, u, v, lens, B, T, H, dk, chunk, left, regime=True, group="regime-" + regime, poison=False)
        if regime == "equal" and chunk == 0:                     # the plain mean of the visible V rows
            vv = qkv.view(B, T, 3, H * dk)[:, :, 2].double()
            mean = torch.stack([vv[b, :lens[b]].mean(0) for b in range(B)])
            assert float((got.cpu().double().view(B, T, -1) - mean.unsqueeze(1)).abs().max()) <= A.TOL


@pytest.mark.parametrize("dk", [64, 128], ids=lambda d: "dk%d" % d)
@pytest.mark.parametrize("T", [50, 128], ids=lambda t: "T%d" % t)
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime_bf16(regime, T, dk):
    """relpos_attention_bf16_kernel (__expf, one-pass softmax): test_relpos_attention_bf16's bound, 1.2e-2 + 1.2e-2 |ref| on valid rows,
    against float64 on the bf16-rounded inputs"""
    B, H = 3, 2
    qkv, p, u, v = A.regime_operands(regime, B, T, H, dk, 710, bf16_rows=True)
    lens = [T, T, T - 9]
    L = torch.tensor(lens, dtype=torch.int32)
    valid = (torch.arange(T).view(1, -1) < L.view(-1, 1)).reshape(-1)
    for chunk, left in ((0, -1), (16, 1)):
        out = ops.relpos_attention_bf16(dev(qkv.to(torch.bfloat16)), dev(p), dev(u), dev(v), dev(L), B, T, H, dk, chunk=chunk, left_chunks=left)
        want = attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left, round_q16=True)
        err = (out.float().cpu().double() - want).abs()[valid]
        e32 = 0.0                                                # (the bound is fixed; the float64 mirror rounds q + u to bf16 itself)
        print("regime-%s bf16 T%d dk%d chunk%d: device err %.3e, bound 1.2e-2 + 1.2e-2 |ref| (max |ref| %.3e)" % (
            regime, T, dk, chunk, float(err.max()), float(want.abs().max())))
        g = A.ERRORS.get("regime-bf16-" + regime, (0.0, 0.0, 0.0))
        A.ERRORS["regime-bf16-" + regime] = (max(g[0], float(err.max())), max(g[1], e32), 1.2e-2)
        assert bool(torch.isfinite(out.float()).all())
        assert bool((err <= 1.2e-2 + 1.2e-2 * want.abs()[valid]).all()), (regime, T, dk, chunk, float(err.max()))


@pytest.mark.parametrize("left", [-1, 2], ids=lambda l: "left%d" % l)
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime_stream(regime, left):
    """relpos_attention_stream_kernel: chunks of 16 over 200 frames (the last chunk holds 8), history from NaN"""
    B, H, dk, C_, n_frames = 2, 2, 64, 16, 200
    nchunks = -(-n_frames // C_)
    T, D = nchunks * C_, H * dk
    qkv, p, u, v = A.regime_operands(regime, B, T, H, dk, 720)
    lens = [n_frames] * B
    want, want32 = A.refs(qkv, p, u, v, lens, B, T, H, dk, C_, left, regime=True)
    cap = T if left < 0 else (left + 1) * C_
    hist = torch.full((B, cap, 2 * D), NAN, device="cuda")
    step, cl = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    rows = []
    for n in range(nchunks):
        step.fill_(n)
        cl.fill_(min(C_, n_frames - n * C_))
        chunk = qkv.view(B, T, 3 * D)[:, n * C_:(n + 1) * C_].reshape(B * C_, 3 * D)
        rows.append(ops.relpos_attention_stream(dev(chunk), hist, dev(p), dev(u), dev(v), cl, step, B, C_, H, dk, left).view(B, C_, D))
    got = torch.cat(rows, 1).reshape(B * T, D)
    valid = (torch.arange(T).view(1, -1) < torch.tensor(lens).view(-1, 1)).reshape(-1)
    A.within("regime-%s stream left%d" % (regime, left), got, want, want32, rows=valid, group="regime-stream-" + regime)


# ================================================================================================ 5. the attention decoder's kernels
def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


def _within(tag, got, r64, r32):
    """tests/test_aed_kernels_gpu.py's yardstick: within max(8 e32, 1e-5) of the float64 mirror, element by element"""
    e32, bound = kref.yardstick(r64, r32)
    err = kref.max_err(got.cpu(), r64)
    print("%s: device err %.3e, e32 %.3e, bound %.3e" % (tag, err, e32, bound))
    g = A.ERRORS.get("aed", (0.0, 0.0, 0.0))
    A.ERRORS["aed"] = (max(g[0], err), max(g[1], e32), max(g[2], bound))
    assert e32 <= 1e-3 * float(r64.abs().max()), tag + ": the float32 yardstick itself is off: fix the inputs"
    assert err <= bound, (tag, err, bound)


def _aed_rows(regime, n_sets, n_keys, n_q, H, dk, g):
    """q [n_q][D] and K | V [n_sets][n_keys][D] whose scores q . k / sqrt(dk) are key_scores (per (set, head)) + a spread of 0.3"""
    D, root = H * dk, math.sqrt(dk)
    W = 4.0 if dk < 64 else 8.0
    q = torch.randn(n_q, H, dk, generator=g) * 0.1
    k, v = torch.randn(n_sets, n_keys, H, dk, generator=g), torch.randn(n_sets, n_keys, H, dk, generator=g)
    s = A.key_scores(regime, n_sets * H, n_keys, g).view(n_sets, H, n_keys).permute(0, 2, 1)
    if regime == "equal":
        q.zero_()
    else:
        if regime == "offset":
            q.zero_()
        q[..., 0] = W
        k[..., 0] = s * (root / W)
    return q.reshape(n_q, D), k.reshape(n_sets, n_keys, D), v.reshape(n_sets, n_keys, D)


AED_DKS = [48, 64]


@pytest.mark.parametrize("dk", AED_DKS, ids=lambda d: "dk%d" % d)
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime_aed_attention(regime, dk):
    """m3_aed_attention: 17 queries over 200 keys, 5 over 50, and 70 causal queries over 70 keys, H = 2"""
    H, g = 2, torch.Generator().manual_seed(800 + dk)
    D = H * dk
    slots, qs, ks, vs, q0, k0 = [(17, 200, 0), (5, 50, 0), (70, 70, 1)], [], [], [], 0, 0
    desc = []
    for n_q, n_k, causal in slots:
        q, k, v = _aed_rows(regime, 1, n_k, n_q, H, dk, g)
        qs.append(q), ks.append(k[0]), vs.append(v[0])
        desc.append((q0, n_q, k0, n_k, causal))
        q0, k0 = q0 + n_q, k0 + n_k
    q, k, v = torch.cat(qs), torch.cat(ks), torch.cat(vs)
    gq, gk, gv, go = G.strided_in(q, ld=D + 8), G.strided_in(k, ld=D + 12), G.strided_in(v, ld=D + 20), G.strided_out(q0, D, ld=D + 9)
    ops.aed_attention(gq.view, gk.view, gv.view, _i32(desc), 70, H, out=go.view)
    torch.cuda.synchronize()
    go.check("aed_attention")
    assert not bool(go.untouched().any())
    r64, wrote = kref.attention(q.double(), k.double(), v.double(), desc, H)
    r32, _ = kref.attention(q, k, v, desc, H)
    assert bool(wrote.all())
    _within("regime-%s aed_attention dk%d" % (regime, dk), G.dense(go.view), r64, r32)


def _search_state(B, N, V, max_steps, pe_rows, D, H, layers=1):
    desc = ops.aed_search_desc(B, N, max_steps, V, D, H, layers, pe_rows)
    return desc, torch.zeros(ops.aed_search_state_size(desc) // 4, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("dk", AED_DKS, ids=lambda d: "dk%d" % d)
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime_search_source(regime, dk):
    """m3_aed_search_attention, source use: B = 2, beam 3, memories of 200 and 50 frames at non-zero rows"""
    B, N, H, mem_len = 2, 3, 2, [200, 50]
    D, R, g = H * dk, B * N, torch.Generator().manual_seed(810 + dk)
    row0 = [60, 5]
    kv = torch.randn(row0[0] + mem_len[0], 2 * D, generator=g)
    qs = []
    for b in range(B):
        q, k, v = _aed_rows(regime, 1, mem_len[b], N, H, dk, g)
        qs.append(q)
        kv[row0[b]:row0[b] + mem_len[b]] = torch.cat([k[0], v[0]], 1)
    q = torch.cat(qs)
    desc, state = _search_state(B, N, 7, 4, 8, D, H)
    ops.aed_search_reset(desc, state, _i32(row0), _i32(mem_len))
    gq, gkv, go = G.strided_in(q, ld=D + 8), G.strided_in(kv, ld=2 * D + 12), G.strided_out(R, D, ld=D + 9)
    ops.aed_search_attention(desc, state, gq.view, gkv.view, go.view, 0)
    torch.cuda.synchronize()
    go.check("aed_search_attention source")
    assert not bool(go.untouched().any())
    r64 = kref.search_source_attention(q.double(), kv.double(), row0, mem_len, N, H)
    r32 = kref.search_source_attention(q, kv, row0, mem_len, N, H)
    _within("regime-%s search source dk%d" % (regime, dk), G.dense(go.view), r64, r32)


@pytest.mark.parametrize("dk", AED_DKS, ids=lambda d: "dk%d" % d)
@pytest.mark.parametrize("regime", A.REGIMES)
def test_regime_search_self(regime, dk):
    """m3_aed_search_attention, self use over 70 steps of a search nobody finishes (kref.walk_case): the keys of position t are the
    K rows of step t, whose scores follow the regime over positions 0 .. 69 (the cache's 64-position tile is crossed); V is random
    per row, so the ancestry matters.  Compared at the steps around the tile edges and the dominant positions."""
    case = kref.walk_case(1, 70)
    B, N, H, steps = case["B"], case["beam"], 2, case["logits"].shape[0]
    D, R, g = H * dk, B * N, torch.Generator().manual_seed(820 + dk)
    desc, state = _search_state(B, N, case["V"], case["max_steps"], case["pe_rows"], D, H)
    ops.aed_search_reset(desc, state, _i32([0] * B), _i32(case["mem_len"]))
    trace = kref.run_search(case, torch.float64)
    q_all, k_all, v_all = _aed_rows(regime, R, steps, steps * R, H, dk, g)
    k_all[:] = k_all[0:1].clone()                                 # every row of a step holds the same K: the score depends on the position alone
    q_all = q_all.view(steps, R, D)
    kv_all = torch.cat([k_all, v_all], 2).transpose(0, 1).contiguous()         # [steps][R][2 D]
    gq, gkv = G.strided_in(q_all.reshape(-1, D), ld=D + 8), G.strided_in(kv_all.reshape(-1, 2 * D), ld=2 * D + 12)
    glog = G.strided_in(case["logits"].reshape(steps * R, case["V"]), ld=case["V"] + 9)
    cache = G.flat_out((1, case["max_steps"], R, 2 * D))
    assert cache.view.numel() * 4 == ops.aed_search_cache_size(desc)
    done = _i32([0] * B)
    outs = {}
    check = (0, 3, 15, 16, 52, 53, 63, 64, 69)
    for s in range(steps):
        go = G.strided_out(R, D, ld=D + 9)
        ops.aed_search_attention(desc, state, gq.view[s * R:(s + 1) * R], gkv.view[s * R:(s + 1) * R], go.view, 0, cache=cache.view)
        if s in check:
            outs[s] = go
        ops.aed_search_prune(desc, state, glog.view[s * R:(s + 1) * R], done)
    torch.cuda.synchronize()
    cache.check("self-attention cache")
    for s in check:
        outs[s].check("aed_search_attention self step %d" % s)
        h = [trace[s][u]["history"] for u in range(B)]
        r64 = kref.search_self_attention(q_all[s].double(), [kv_all[t].double() for t in range(s + 1)], h, s, N, H)
        r32 = kref.search_self_attention(q_all[s], [kv_all[t] for t in range(s + 1)], h, s, N, H)
        _within("regime-%s search self dk%d step %d" % (regime, dk, s), G.dense(outs[s].view), r64, r32)

