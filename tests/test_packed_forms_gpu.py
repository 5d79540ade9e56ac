"""The packed-row and bf16-row operand forms of the block kernels, called directly (include/m3asr.h "Packed rows").

Ragged batches (packed_rows) and the 16-bit modes of long batches run every block kernel in a second operand form: a device-side
count of live rows on the GEMMs and the router, the valid frames per utterance on the implicit conv, a row plan on attention and
the depthwise conv, bf16 copies and row statistics on LayerNorm.  Until now only whole-encoder comparisons reached them.  Here
each form is held, on guarded operands (tests/guarded.py), to three things: the SAME operator's plain launch bit for bit on the
rows it owns, an fp64 reference (tests/packed_ref.py) at the bound of the existing direct test of the kernel, and "writes nothing
it does not own": rows behind the live count, a packed neighbour's frames and every guard keep their fill pattern.  The live
counts sit on, one below and one above the 16 / 64 / 128-row tile edges, at 0 and at the full row count.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded as G
import packed_ref as R
from m3asr import ops, _lib
from m3asr._lib import M3Error
from m3asr.plan import fold_layernorm


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.cuda().contiguous()


def i32(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32)


def close(got, want, rtol, atol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    print("%s max abs err %.3e (max |ref| %.3e, bound %.1e / %.1e)" % (what, float(err.max()) if err.numel() else 0.0,
                                                                        float(want.abs().max()) if want.numel() else 0.0, rtol, atol))
    assert bool((err <= bound).all()), "%s max abs err %.3e (max |ref| %.3e), worst excess %.3e" % (
        what, float(err.max()), float(want.abs().max()), float((err - bound).max()))


def plan_dev(lens, T):
    """the reference plan of (lens, T) on the device: (lens, row0, pad_of, P) -- independent of m3_pack_plan, which has its own test"""
    len_out, row0, pad_of, P = R.row_plan(lens, T)
    return dev(i32(len_out)), dev(i32(row0)), dev(i32(pad_of)), P


# ================================================================================================ row plan and unpack
PT = 9
PLAN_LENS = {"B1": [5], "all_empty": [0, 0, 0], "all_full": [PT, PT, PT], "mixed": [1, 0, PT, 3, 0],
             "clamped": [PT + 4, -2, 3, PT, -1, 0, 2 * PT], "B1024": list(np.random.RandomState(7).randint(0, PT + 1, size=1024))}
PLAN_FEAT = {"6_7_11": [6, 7, 11], "edges": [4, 6, 7, 11, 3, 43, 39, 0, -5, 200], "B1024": list(np.random.RandomState(8).randint(0, 48, size=1024))}


def _check_plan(lens, feat):
    B = len(feat if feat is not None else lens)
    want_len, want_row0, want_pad, P = R.row_plan(lens, PT, feat_len=feat)
    g_row0, g_pad = G.flat_out((B + 1,), torch.int32), G.flat_out((B * PT,), torch.int32)
    if feat is None:
        g_len = G.flat_in(i32(lens), int_guard=PT)                # an input: a consumed guard is a valid length, and a wrong plan
        ops.pack_plan(g_len.view, PT, row0=g_row0.view, pad_of=g_pad.view)
    else:
        g_len = G.flat_out((B,), torch.int32)                     # an output: the subsampled lengths
        g_feat = G.flat_in(i32(feat), int_guard=43)
        ops.pack_plan(g_len.view, PT, feat_len=g_feat.view, row0=g_row0.view, pad_of=g_pad.view)
        g_len.check("len")
    torch.cuda.synchronize()
    g_row0.check("row0")
    g_pad.check("pad_of")
    assert g_len.view.cpu().tolist() == want_len.tolist()
    assert g_row0.view.cpu().tolist() == want_row0.tolist()
    got_pad = g_pad.view.cpu().tolist()
    assert got_pad[:P] == want_pad[:P].tolist()
    assert got_pad[P:] == [-1] * (B * PT - P)
    return P


@pytest.mark.parametrize("name", list(PLAN_LENS))
def test_pack_plan_from_lengths(name):
    """pack_plan_kernel: row0 and pad_of exactly, lengths untouched; B = 1, P = 0, P = B * T, empty utterances between live ones,
    the B = 1024 limit, and lengths above T and below 0 (clamped for the rows only)."""
    P = _check_plan(PLAN_LENS[name], None)
    assert {"all_empty": P == 0, "all_full": P == 3 * PT, "clamped": P == PT + 3 + PT + PT}.get(name, True)


@pytest.mark.parametrize("name", list(PLAN_FEAT))
def test_pack_plan_from_feature_lengths(name):
    """... with the subsampled lengths formed in the same launch (C int arithmetic: 6, 7, 11 raw frames -> 1, 1, 2 frames; 4 -> 0;
    200 -> 49, stored as computed and clamped to T = 9 rows)."""
    _check_plan(None, PLAN_FEAT[name])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_unpack_rows(n):
    """unpack_rows_kernel: live rows are exact copies, the rest zeros; P = 0 and P = B * T included"""
    for lens in ([1, 0, PT, 3, 0], [0, 0, 0], [PT, PT, PT], [5]):
        B = len(lens)
        _, row0, _, P = R.row_plan(lens, PT)
        rows = rnd(max(P, 1), n, seed=n)                          # (P = 0: one row that no frame maps to)
        g_in = G.flat_in(rows)
        g_out = G.flat_out((B * PT, n))
        ops.unpack_rows(g_in.view, dev(i32(row0)), B, PT, out=g_out.view)
        torch.cuda.synchronize()
        g_out.check("unpack n=%d %s" % (n, lens))
        assert G.same_bits(g_out.view.cpu(), R.unpack(rows, row0, B, PT)), (n, lens)


# ================================================================================================ GEMM live rows (m_dev)
def _edges(M):
    return sorted({p for p in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, M - 1, M) if 0 <= p <= M})


def _check_live_rows(gy, y_full, P, M, tag):
    """The contract of a live-row launch on a pattern-filled output: every row is written whole or not at all; the unwritten rows
    are a suffix that starts at a multiple of 16 above P and no later than the first multiple of 128 above P (128 = the largest
    row tile of the dense family: the skip must really happen); every written row holds the plain launch's bits."""
    gy.check(tag)
    unt = gy.untouched()
    row_all, row_any = unt.all(1), unt.any(1)
    assert bool((row_all == row_any).all()), tag + ": a row is written in part"
    first = int(torch.nonzero(row_all)[0]) if bool(row_all.any()) else M
    assert bool(row_all[first:].all()), tag + ": unwritten rows are not a suffix"
    assert first > P or first == M, tag + ": row %d <= P is not written" % first
    assert first == M or first % 16 == 0, tag + ": the unwritten rows start at %d" % first
    limit = (P // 128 + 1) * 128
    if limit < M:
        assert first <= limit, tag + ": rows up to %d are written, no tile behind P = %d is skipped" % (first, P)
    assert G.same_bits(G.dense(gy.view[:first]), y_full[:first]), tag + ": a written row differs from the plain launch"
    return first


def _live_rows_gemm(kernel, M, N, K, *, w16=False, a16=False, act=_lib.ACT_NONE, mask=None, ln_stats=False, tol=2e-5, Ps=None):
    """One kernel of the dense family under m_dev, for every P in Ps.  mask: None / "in" / "out" -- the engine's packed form of the
    masks, row_len = the live count itself and rows_per_batch = M, so rows >= P are the padding (mask "out" with a residual)."""
    glu = act == _lib.ACT_GLU
    n_out = N // 2 if glu else N
    a = rnd(M, K, seed=1)
    if a16:
        a = a.to(torch.bfloat16)
    w, b = rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    res = rnd(M, n_out, seed=4) if mask == "out" else None
    kw = dict(act=act)
    w_dev, b_dev = (w.to(torch.bfloat16) if w16 else w), b
    ad = R.bf16(a) if w16 else a.double()                         # bf16 weights: A is rounded to bf16 at the MFMA input
    if ln_stats:                                                  # folded LayerNorm from the producer's row statistics (LDS-DMA kernel)
        ga, be = rnd(K, seed=5) * 0.2 + 1.0, rnd(K, seed=6, scale=0.1)
        f = fold_layernorm(w, b, ga, be)
        w_dev, b_dev = f["ln.weight"].to(torch.bfloat16), f["ln.bias"]
        wsum = w_dev.double().sum(1).float()
        x64 = a.double()
        st = torch.zeros(M, 4, 2)                                 # total in part 0, zeros elsewhere: what m3_layer_norm_ex leaves
        st[:, 0, 0], st[:, 0, 1] = x64.sum(1).float(), (x64 * x64).sum(1).float()
        mu, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
        z = (ad @ w_dev.double().t() - mu * wsum.double()) / torch.sqrt(var + 1e-12) + b_dev.double()
        kw.update(ln_folded=(dev(wsum), None, 1e-12), ln_stats=dev(st))
    else:
        z = ad @ (R.bf16(w) if w16 else w.double()).t() + b.double()
    wd_, bd_ = dev(w_dev), dev(b_dev)
    ga_ = G.strided_in(a)
    res_d = dev(res) if res is not None else None
    y_plain = None
    for P in (Ps if Ps is not None else _edges(M)):
        tag = "%s M=%d N=%d K=%d P=%d" % (kernel, M, N, K, P)
        count = G.flat_in(i32([P]), int_guard=M)                  # (a consumed guard: every row live, caught by the suffix bound)
        pkw = dict(kw)
        live = (torch.arange(M) < P).view(M, 1)
        zz = z
        if mask == "in":                                          # masked_fill(0) of the input rows: the bias alone
            pkw.update(lens=count.view, rows_per_batch=M, mask_in=True)
            zz = torch.where(live, z, b.double().expand_as(z))
        if glu:
            zz = zz[:, :n_out] * torch.sigmoid(zz[:, n_out:])
        if mask == "out":
            pkw.update(lens=count.view, rows_per_batch=M, mask_out=True, resid=res_d)
            zz = torch.where(live, zz, torch.zeros_like(zz)) + res.double()
        assert ops.linear_kernel(ga_.view, wd_, bd_, live_rows=count.view, **pkw) == kernel, tag
        if mask or y_plain is None:                               # the same descriptor without the count (a mask reads the count)
            y_plain = ops.linear(ga_.view, wd_, bd_, **pkw)
        y_full = y_plain
        gy = G.strided_out(M, n_out)
        ops.linear(ga_.view, wd_, bd_, out=gy.view, live_rows=count.view, **pkw)
        # NaN in every A row above P must not reach a row <= P
        a_nan = a.clone()
        a_nan[P + 1:] = float("nan")
        gn = G.strided_out(M, n_out)
        ops.linear(G.strided_in(a_nan).view, wd_, bd_, out=gn.view, live_rows=count.view, **pkw)
        torch.cuda.synchronize()
        first = _check_live_rows(gy, y_full, P, M, tag)
        gn.check(tag + " (NaN rows)")
        upto = min(P + 1, M)
        assert G.same_bits(G.dense(gn.view[:upto]), y_full[:upto]), tag + ": NaN above P reached a live row"
        assert bool(gn.untouched()[first:].all()), tag + " (NaN rows): the skipped rows differ"
        if mask or P == 0:
            close(y_full, zz, tol, tol, tag)


# tolerances: the bound the existing direct test of the same kernel holds, cited per case
def test_live_rows_skinny_f32():
    """gemm_f32_kernel, 16-row tiles; bound of test_linear_plain / test_linear_epilogues (2e-5)"""
    _live_rows_gemm("gemm_f32_kernel", 200, 64, 64, tol=2e-5)
    _live_rows_gemm("gemm_f32_kernel", 200, 128, 64, act=_lib.ACT_GLU, tol=2e-5, Ps=[0, 15, 16, 17, 199, 200])
    _live_rows_gemm("gemm_f32_kernel", 200, 64, 64, mask="in", tol=2e-5, Ps=[0, 15, 16, 17, 199, 200])
    _live_rows_gemm("gemm_f32_kernel", 200, 64, 64, mask="out", tol=2e-5, Ps=[0, 15, 16, 17, 199, 200])


def test_live_rows_skinny_bf16w():
    """gemm_bf16w_kernel, 32-row tiles at 200 rows; bound of test_linear_bf16_plain (2e-5)"""
    _live_rows_gemm("gemm_bf16w_kernel", 200, 64, 64, w16=True, tol=2e-5)


def test_live_rows_tiled_f32_64():
    """gemm_f32_tiled_kernel, 64-row tiles (384 x 2048: 192 tiles of 64 x 64, 48 of 128 x 128); bound of test_linear_tiled_plain /
    test_linear_tiled_epilogues (3e-5)"""
    _live_rows_gemm("gemm_f32_tiled_kernel", 384, 2048, 64, tol=3e-5)
    _live_rows_gemm("gemm_f32_tiled_kernel", 384, 4096, 64, act=_lib.ACT_GLU, tol=3e-5, Ps=[0, 63, 64, 65, 383, 384])
    _live_rows_gemm("gemm_f32_tiled_kernel", 384, 2048, 64, mask="in", tol=3e-5, Ps=[0, 63, 64, 65, 383, 384])
    _live_rows_gemm("gemm_f32_tiled_kernel", 384, 2048, 64, mask="out", tol=3e-5, Ps=[0, 63, 64, 65, 383, 384])


def test_live_rows_tiled_f32_128():
    """gemm_f32_tiled_kernel, 128-row tiles (1664 x 2048: 208 tiles of 128 x 128); bound of test_linear_tiled_plain (3e-5)"""
    _live_rows_gemm("gemm_f32_tiled_kernel", 1664, 2048, 64, tol=3e-5)


@pytest.mark.parametrize("a16", [False, True], ids=["a_f32", "a_bf16"])
def test_live_rows_tiled_bf16w(a16):
    """gemm_bf16w_tiled_kernel, 64-row tiles, fp32 and bf16 A; bound of test_linear_bf16_epilogues at its tiled shape (3e-5)"""
    _live_rows_gemm("gemm_bf16w_tiled_kernel", 384, 2048, 128, w16=True, a16=a16, tol=3e-5)


def test_live_rows_dma_bf16():
    """gemm_bf16_dma_kernel, 128-row tiles; bound of test_linear_bf16_dma_plain_and_residual (2e-5), and for the folded LayerNorm
    from ln_stats that of test_linear_bf16_dma_epilogues (2e-3)"""
    _live_rows_gemm("gemm_bf16_dma_kernel", 4096, 128, 64, w16=True, a16=True, tol=2e-5)
    _live_rows_gemm("gemm_bf16_dma_kernel", 4096, 128, 128, w16=True, a16=True, ln_stats=True, tol=2e-3, Ps=[0, 127, 128, 129, 4095, 4096])


def test_live_rows_router():
    """moe_router_kernel at S = 200, E = 32 (16-row tiles): logits and xn under the live count; bounds of test_moe_router"""
    S, E, De, D = 200, 32, 64, 128
    emb, x = rnd(S, De, seed=1), rnd(S, D, seed=2) * 1.7 + 0.4
    wr, b = rnd(E, De + D, seed=3, scale=0.5), rnd(E, seed=4)
    ga, be = rnd(D, seed=5, scale=0.3) + 1.0, rnd(D, seed=6, scale=0.2)
    eps = 1e-12
    want_xn = F.layer_norm(x.double(), (D,), ga.double(), be.double(), eps)
    want = torch.cat([emb.double(), want_xn], -1) @ wr.double().t() + b.double()
    ln = (dev(ga), dev(be), eps)
    g_emb, g_x = G.strided_in(emb), G.strided_in(x)
    y_full, xn_full = ops.moe_router(g_emb.view, g_x.view, dev(wr), ln, bias=dev(b))
    close(xn_full, want_xn, 2e-5, 2e-5, "router xn")
    close(y_full, want, 2e-5, 2e-4, "router logits")
    for P in _edges(S):
        tag = "moe_router_kernel S=%d P=%d" % (S, P)
        count = G.flat_in(i32([P]), int_guard=S)
        gy, gxn = G.strided_out(S, E), G.strided_out(S, D)
        ops.moe_router(g_emb.view, g_x.view, dev(wr), ln, bias=dev(b), out=gy.view, xn_out=gxn.view, live_rows=count.view)
        x_nan, e_nan = x.clone(), emb.clone()
        x_nan[P + 1:], e_nan[P + 1:] = float("nan"), float("nan")
        gyn, gxnn = G.strided_out(S, E), G.strided_out(S, D)
        ops.moe_router(G.strided_in(e_nan).view, G.strided_in(x_nan).view, dev(wr), ln, bias=dev(b), out=gyn.view, xn_out=gxnn.view,
                       live_rows=count.view)
        torch.cuda.synchronize()
        first = _check_live_rows(gy, y_full, P, S, tag + " logits")
        assert _check_live_rows(gxn, xn_full, P, S, tag + " xn") == first
        assert first == min((P // 16 + 1) * 16, S) or first == S, tag      # its row tile has 16 rows
        upto = min(P + 1, S)
        gyn.check(tag + " (NaN rows) logits")
        gxnn.check(tag + " (NaN rows) xn")
        assert G.same_bits(G.dense(gyn.view[:upto]), y_full[:upto]) and G.same_bits(G.dense(gxnn.view[:upto]), xn_full[:upto]), tag


# ================================================================================================ implicit conv, valid frames (conv_len)
# the smallest shapes the tiled kernels take with four utterances (tests/test_packed_forms_host.py test_conv2d_kernel_query):
# F2 = 65 output columns per frame, so 64-row tiles start inside frames and 2600 / 1300 rows per utterance put tiles across utterances
@pytest.mark.parametrize("w16,T1,F1,C,kernel", [(False, 81, 131, 64, "gemm_f32_tiled_kernel"), (True, 41, 131, 128, "gemm_bf16w_tiled_kernel")],
                         ids=["f32", "bf16w"])
def test_conv2d_valid_frames(w16, T1, F1, C, kernel):
    B, tile = 4, 64
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    per_utt, M = T2 * F2, B * T2 * F2
    assert ops.conv2d_kernel(B, T1, F1, C, _lib.ACT_RELU, w16) == kernel
    assert per_utt % tile != 0 and M % tile != 0                                     # tiles cross utterances; the last one is partial
    x = torch.rand(B, T1, F1, C, generator=torch.Generator().manual_seed(1))
    w2, b2 = rnd(C, C, 3, 3, seed=4, scale=(9 * C) ** -0.5), rnd(C, seed=5, scale=0.1)
    w_dev = dev(w2.permute(0, 2, 3, 1).contiguous())
    if w16:
        w_dev = w_dev.to(torch.bfloat16)
    gx = G.flat_in(x)
    y_full = ops.conv2d_frames(gx.view, w_dev, dev(b2)).view(M, C)
    xd, wd = (R.bf16(x), R.bf16(w2)) if w16 else (x.double(), w2.double())
    want = F.relu(F.conv2d(xd.permute(0, 3, 1, 2), wd, b2.double(), stride=2)).permute(0, 2, 3, 1).reshape(M, C)
    close(y_full, want, 3e-5, 3e-5, kernel + " conv")                               # bound of test_subsampling_convs (conv2)
    # frames: all, none, one, and a count that puts a 64-row tile edge inside the utterance's valid rows and another inside
    # its padded rows (7 frames = 455 rows: tile edges at every 64 rows of the utterance's 2600 / 1300)
    for frames in ([T2, 0, 1, 7], [0, T2, 7, 1], [T2 + 5, -1, T2 - 1, T2]):
        tag = "%s frames=%s" % (kernel, frames)
        gf = G.flat_in(i32(frames), int_guard=T2)
        gy = G.flat_out((M, C))
        ops.conv2d_frames(gx.view, w_dev, dev(b2), frames=gf.view, out=gy.view.view(B, T2, F2, C))
        torch.cuda.synchronize()
        gy.check(tag)
        unt = gy.untouched()
        row_all = unt.all(1)
        assert bool((row_all == unt.any(1)).all()), tag + ": a row is written in part"
        written = ~row_all
        assert G.same_bits(gy.view[written], y_full[written]), tag + ": a written row differs from the launch without frames"
        row_all = row_all.cpu()
        m = torch.arange(M)
        b_of, t_of = m // per_utt, (m % per_utt) // F2
        valid = t_of < torch.tensor(frames).clamp(0, T2)[b_of]
        assert not bool(row_all[valid].any()), tag + ": a row of a valid frame is not written"
        # tile by tile: a tile is skipped as a whole or not at all; one that spans two utterances never; one inside an utterance
        # whose first row is a padded frame is (that is the skip, and the 0-frame utterance has whole tiles of them)
        skipped_in = {b: 0 for b in range(B)}
        for m0 in range(0, M, tile):
            m1 = min(m0 + tile, M) - 1
            rows = row_all[m0:m1 + 1]
            assert bool(rows.all()) or not bool(rows.any()), tag + ": tile at row %d is written in part" % m0
            b0, b1 = m0 // per_utt, m1 // per_utt
            expect_skip = b0 == b1 and (m0 - b0 * per_utt) // F2 >= frames[b0]
            assert bool(rows.all()) == expect_skip, tag + ": tile at row %d (utterances %d..%d) %s" % (
                m0, b0, b1, "is not skipped" if expect_skip else "is skipped")
            skipped_in[b0] += int(expect_skip)
        empty = [b for b in range(B) if frames[b] <= 0]
        assert all(skipped_in[b] >= per_utt // tile - 1 for b in empty), tag


# ================================================================================================ packed attention
ATT_T = 33
ATT_LENS = {"ragged": [16, 1, 0, 17, 15, 33], "one": [33], "empty_first": [0, 33]}


def _att_operands(B, H, dk, bf16_rows):
    D = H * dk
    qkv, p = rnd(B * ATT_T, 3 * D, seed=1), rnd(ATT_T, D, seed=2)
    if bf16_rows:
        qkv = qkv.to(torch.bfloat16)
    return qkv, p, rnd(H, dk, seed=3, scale=0.3), rnd(H, dk, seed=4, scale=0.3)


@pytest.mark.parametrize("chunk,left", [(0, -1), (16, 2)], ids=["full", "chunk16_left2"])
@pytest.mark.parametrize("name", list(ATT_LENS))
@pytest.mark.parametrize("dk", [64, 128])
def test_packed_attention_f32(dk, name, chunk, left):
    """relpos_attention_kernel with row0 (and out_bf16).  Lengths 16 / 17 / 15 / 33 sit on, above and below the 16-row query tile,
    a one-frame and an empty utterance lie between them; tolerance of test_relpos_attention (3e-5)."""
    lens, T, H = ATT_LENS[name], ATT_T, 2
    B, D = len(lens), 2 * dk
    qkv, p, u, v = _att_operands(B, H, dk, False)
    L, row0, pad_of, P = plan_dev(lens, T)
    gp = G.strided_in(p)
    args = (gp.view, dev(u), dev(v), L, B, T, H, dk)
    out_pad = ops.relpos_attention_packed(dev(qkv), *args, out=torch.empty(B * T, D, device="cuda"), chunk=chunk, left_chunks=left)
    assert G.same_bits(out_pad, ops.relpos_attention(dev(qkv), *args, chunk=chunk, left_chunks=left))     # row0 = NULL: the padded entry
    idx = pad_of[:P].long()
    packed = qkv[idx.cpu()]
    gq, go, gb = G.strided_in(packed), G.strided_out(P, D), G.strided_out(P, D, torch.bfloat16)
    ops.relpos_attention_packed(gq.view, *args, out=go.view, row0=row0, chunk=chunk, left_chunks=left)
    ops.relpos_attention_packed(gq.view, *args, out=gb.view, row0=row0, chunk=chunk, left_chunks=left)
    torch.cuda.synchronize()
    tag = "packed attention dk=%d %s chunk=%d" % (dk, name, chunk)
    go.check(tag)                                               # rows at and above P are guard rows: untouched
    gb.check(tag + " out_bf16")
    assert not bool(go.untouched().any()) and not bool(gb.untouched().any()), tag + ": a live row is not written"
    got = G.dense(go.view)
    assert G.same_bits(got, out_pad[idx]), tag + ": packed rows differ from the padded call"
    assert G.same_bits(G.dense(gb.view), got.to(torch.bfloat16)), tag + ": the bf16 output is not the rounded fp32 output"
    close(got, R.packed_attention_ref(packed, p, u, v, lens, row0.cpu().numpy(), T, H, dk, chunk, left), 3e-5, 3e-5, tag)
    # NaN in every row an utterance does not own: its rows stay what they were
    r0 = row0.cpu().tolist()
    for b in range(B):
        if r0[b + 1] == r0[b]:
            continue
        alone = torch.full_like(packed, float("nan"))
        alone[r0[b]:r0[b + 1]] = packed[r0[b]:r0[b + 1]]
        gn = G.strided_out(P, D)
        ops.relpos_attention_packed(G.strided_in(alone).view, *args, out=gn.view, row0=row0, chunk=chunk, left_chunks=left)
        torch.cuda.synchronize()
        gn.check(tag + " (NaN neighbours)")
        assert G.same_bits(G.dense(gn.view[r0[b]:r0[b + 1]]), got[r0[b]:r0[b + 1]]), tag + ": utterance %d read a row it does not own" % b


@pytest.mark.parametrize("chunk,left", [(0, -1), (16, 2)], ids=["full", "chunk16_left2"])
@pytest.mark.parametrize("name", list(ATT_LENS))
@pytest.mark.parametrize("dk", [64, 128])
def test_packed_attention_bf16_rows(dk, name, chunk, left):
    """relpos_attention_bf16_kernel (T <= 128) with row0; tolerance of test_relpos_attention_bf16 (1.2e-2)"""
    lens, T, H = ATT_LENS[name], ATT_T, 2
    B, D = len(lens), 2 * dk
    qkv, p, u, v = _att_operands(B, H, dk, True)
    L, row0, pad_of, P = plan_dev(lens, T)
    gp = G.strided_in(p)
    args = (gp.view, dev(u), dev(v), L, B, T, H, dk)
    out_pad = ops.relpos_attention_bf16(dev(qkv), *args, chunk=chunk, left_chunks=left)
    idx = pad_of[:P].long()
    packed = qkv[idx.cpu()]
    gq, go = G.strided_in(packed), G.strided_out(P, D, torch.bfloat16)
    ops.relpos_attention_packed(gq.view, *args, out=go.view, row0=row0, chunk=chunk, left_chunks=left)
    torch.cuda.synchronize()
    tag = "packed attention (bf16 rows) dk=%d %s chunk=%d" % (dk, name, chunk)
    go.check(tag)
    assert not bool(go.untouched().any()), tag + ": a live row is not written"
    got = G.dense(go.view)
    assert G.same_bits(got, out_pad[idx]), tag + ": packed rows differ from the padded call"
    want = R.packed_attention_ref(packed.float(), p, u, v, lens, row0.cpu().numpy(), T, H, dk, chunk, left, bf16_rows=True)
    close(got.float(), want, 1.2e-2, 1.2e-2, tag)
    r0 = row0.cpu().tolist()
    for b in range(B):
        if r0[b + 1] == r0[b]:
            continue
        alone = torch.full_like(packed, float("nan"))
        alone[r0[b]:r0[b + 1]] = packed[r0[b]:r0[b + 1]]
        gn = G.strided_out(P, D, torch.bfloat16)
        ops.relpos_attention_packed(G.strided_in(alone).view, *args, out=gn.view, row0=row0, chunk=chunk, left_chunks=left)
        torch.cuda.synchronize()
        gn.check(tag + " (NaN neighbours)")
        assert G.same_bits(G.dense(gn.view[r0[b]:r0[b + 1]]), got[r0[b]:r0[b + 1]]), tag + ": utterance %d read a row it does not own" % b


# ================================================================================================ packed depthwise conv
DW_T = 20
DW_LENS = {"ragged": [1, 0, 7, 8, 20], "all_full": [20, 20]}      # all_full: P = B * T, the pad row is row B * T


def _dw_operands(B, D, K, glu):
    z = rnd(B * DW_T, 2 * D if glu else D, seed=1)
    pad_row = rnd(2 * D if glu else D, seed=8)
    w_kc, bias = rnd(K, D, seed=2, scale=0.3), rnd(D, seed=3, scale=0.1)
    return z, pad_row, w_kc, bias, rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1), rnd(D, seed=7)


@pytest.mark.parametrize("form", ["symmetric", "causal", "glu", "glu_sigmoided"])
@pytest.mark.parametrize("name", list(DW_LENS))
@pytest.mark.parametrize("D,K", [(64, 15), (512, 15), (512, 7), (64, 7)])
def test_packed_dwconv(D, K, name, form):
    """dwconv_ln_silu_kernel with pad_of / row0 / row_len (and out_bf16), in every form dwconv_glu_in_supports admits; the others are
    refused.  Tolerance of test_dwconv_ln_silu (2e-5)."""
    lens, T = DW_LENS[name], DW_T
    B = len(lens)
    glu = form.startswith("glu")
    z, pad_row, w_kc, bias, gamma, beta, fill = _dw_operands(B, D, K, glu)
    if form == "glu_sigmoided":                                 # the gate columns hold sigmoid(gate) already
        z[:, D:], pad_row[D:] = torch.sigmoid(z[:, D:]), torch.sigmoid(pad_row[D:])
    L, row0, pad_of, P = plan_dev(lens, T)
    idx = pad_of[:P].long().cpu()
    packed = torch.cat([z[idx], pad_row.view(1, -1)])           # P live rows, then the pad row
    live = (torch.arange(T).view(1, -1) < torch.tensor(lens).view(-1, 1)).reshape(-1, 1)
    z_pad = torch.where(live, z, pad_row.view(1, -1).expand_as(z))   # the padded layout: frames >= len hold the pad row
    wd, bd, gd, bed = dev(w_kc), dev(bias), dev(gamma), dev(beta)
    left_fill = dev(fill) if form == "causal" else None
    kw = dict(left_fill=left_fill, glu=glu, gate_sigmoided=form == "glu_sigmoided")
    gz = G.strided_in(packed) if glu else G.flat_in(packed)
    plan = (pad_of, row0, L)
    tag = "packed dwconv D=%d K=%d %s %s" % (D, K, name, form)
    if glu and not (256 <= D <= 1024):                          # dwconv_glu_in_supports: refused, nothing launched
        with pytest.raises(M3Error, match="GLU on load"):
            ops.dwconv_ln_silu_packed(gz.view, wd, bd, gd, bed, 1e-5, B, T, torch.empty(P, D, device="cuda"), plan=plan, **kw)
        return
    # the padded launch: the single entry of the form where one exists, else the same entry without a plan
    zp = dev(z_pad)
    if form == "symmetric":
        out_pad = ops.dwconv_ln_silu(zp, wd, bd, gd, bed, 1e-5, B, T)
    elif form == "causal":
        out_pad = ops.dwconv_ln_silu_causal(zp, wd, bd, gd, bed, 1e-5, left_fill, B, T)
    elif form == "glu":
        out_pad = ops.dwconv_glu_ln_silu(zp, wd, bd, gd, bed, 1e-5, B, T)
    else:
        out_pad = torch.empty(B * T, D, device="cuda")
    same_entry = ops.dwconv_ln_silu_packed(zp, wd, bd, gd, bed, 1e-5, B, T, torch.empty(B * T, D, device="cuda"), **kw)
    if form != "glu_sigmoided":
        assert G.same_bits(same_entry, out_pad), tag + ": the entry without a plan is not the padded entry"
    out_pad = same_entry
    go = G.flat_out((P, D))
    ops.dwconv_ln_silu_packed(gz.view, wd, bd, gd, bed, 1e-5, B, T, go.view, plan=plan, **kw)
    torch.cuda.synchronize()
    go.check(tag)                                               # rows >= P are guard: untouched
    assert not bool(go.untouched().any()), tag + ": a live row is not written"
    got = go.view.clone()
    assert G.same_bits(got, out_pad[idx.cuda()]), tag + ": packed rows differ from the padded launch"
    if glu:
        val = lambda t: (t[..., :D].double() * (t[..., D:].double() if form == "glu_sigmoided" else torch.sigmoid(t[..., D:].double())))
        z_ref, pad_ref = val(packed[:P]), val(pad_row)
    else:
        z_ref, pad_ref = packed[:P], pad_row
    want = R.packed_dwconv_ref(z_ref, pad_ref, w_kc, bias, gamma, beta, 1e-5, lens, row0.cpu().numpy(), T,
                               left_fill=fill if form == "causal" else None)
    close(got, want, 2e-5, 2e-5, tag)
    if not glu:                                                 # bf16 output: the rounded fp32 result, packed and padded
        gb = G.flat_out((P, D), torch.bfloat16)
        ops.dwconv_ln_silu_packed(gz.view, wd, bd, gd, bed, 1e-5, B, T, gb.view, plan=plan, **kw)
        pad16 = ops.dwconv_ln_silu_packed(zp, wd, bd, gd, bed, 1e-5, B, T, torch.empty(B * T, D, dtype=torch.bfloat16, device="cuda"), **kw)
        torch.cuda.synchronize()
        gb.check(tag + " out_bf16")
        assert G.same_bits(gb.view.clone(), got.to(torch.bfloat16)), tag + ": the bf16 output is not the rounded fp32 output"
        assert G.same_bits(gb.view.clone(), pad16[idx.cuda()]), tag + ": bf16 packed rows differ from the padded launch"
    else:
        with pytest.raises(M3Error, match="GLU on load"):       # the GLU-on-load forms have no bf16 output
            ops.dwconv_ln_silu_packed(gz.view, wd, bd, gd, bed, 1e-5, B, T, torch.empty(P, D, dtype=torch.bfloat16, device="cuda"), plan=plan, **kw)
    if name == "all_full" and form != "causal":                 # every frame live: the pad row is never a tap
        nan_pad = packed.clone()
        nan_pad[P] = float("nan")
        gn = G.flat_out((P, D))
        ops.dwconv_ln_silu_packed((G.strided_in(nan_pad) if glu else G.flat_in(nan_pad)).view, wd, bd, gd, bed, 1e-5, B, T, gn.view, plan=plan, **kw)
        torch.cuda.synchronize()
        gn.check(tag + " (NaN pad row)")
        assert G.same_bits(gn.view.clone(), got), tag + ": an utterance of length T read the pad row"


def test_packed_dwconv_causal_glu_is_refused():
    """GLU on load is the symmetric conv's alone (check_dwconv)"""
    B, T, D, K = 2, DW_T, 512, 15
    z, pad_row, w_kc, bias, gamma, beta, fill = _dw_operands(B, D, K, True)
    L, row0, pad_of, P = plan_dev([20, 20], T)
    with pytest.raises(M3Error, match="GLU on load"):
        ops.dwconv_ln_silu_packed(dev(torch.cat([z, pad_row.view(1, -1)])), dev(w_kc), dev(bias), dev(gamma), dev(beta), 1e-5, B, T,
                                  torch.empty(P, D, device="cuda"), plan=(pad_of, row0, L), left_fill=dev(fill), glu=True)


# ================================================================================================ LayerNorm extras, row statistics
def _check_stats(stats, xb, tag):
    """stats [rows][4][2] against the fp64 sums of the bf16 values: parts 1..3 exact zeros, part 0 within the worst case of an
    fp32 sum of D terms in any order (packed_ref.row_stats_ref)"""
    st = stats.cpu().double()
    assert bool((stats.cpu()[:, 1:] == 0).all()) and not bool(torch.signbit(stats.cpu()[:, 1:]).any()), tag + ": parts 1..3 are not zeros"
    s1, s2, b1, b2 = R.row_stats_ref(xb.cpu())
    e1, e2 = (st[:, 0, 0] - s1).abs(), (st[:, 0, 1] - s2).abs()
    print("%s sum err %.3e (bound %.3e), sum of squares err %.3e (bound %.3e)" % (tag, float(e1.max()), float(b1.min()), float(e2.max()), float(b2.min())))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), tag
    return b1, b2


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [4, 256, 260, 2048])
def test_layer_norm_extras(D, rows):
    """layernorm_kernel's bf16 copy, row statistics and second LayerNorm, over its instantiations and the 4-rows-per-work-group
    tail; y2 at test_layer_norm_sweep's (0, 1) bound (1e-5 / 1e-5)"""
    x = rnd(rows, D, seed=D + rows)
    ga, be = rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1)
    ga2, be2 = rnd(D, seed=6) * 0.2 + 1.0, rnd(D, seed=7, scale=0.1)
    gad, bed, ga2d, be2d = dev(ga), dev(be), dev(ga2), dev(be2)
    tag = "layer_norm_ex D=%d rows=%d" % (D, rows)
    for eps, eps2 in ((1e-5, 1e-12), (1e-12, 1e-5)):
        y_plain = ops.layer_norm(dev(x), gad, bed, eps)
        gx = G.flat_in(x)
        gy, gb, gs, g2 = G.flat_out((rows, D)), G.flat_out((rows, D), torch.bfloat16), G.flat_out((rows, 4, 2)), G.flat_out((rows, D))
        ops.layer_norm_ex(gx.view, gad, bed, eps, y=gy.view, y_bf16=gb.view, y_stats=gs.view, ln2=(ga2d, be2d, eps2), y2=g2.view)
        torch.cuda.synchronize()
        for g, n in ((gy, "y"), (gb, "y_bf16"), (gs, "y_stats"), (g2, "y2")):
            g.check(tag + " " + n)
            assert not bool(g.untouched().any()), tag + ": %s has unwritten elements" % n
        y = gy.view.clone()
        assert G.same_bits(y, y_plain), tag + ": y is not m3_layer_norm's"
        assert G.same_bits(gb.view.clone(), y.to(torch.bfloat16)), tag + ": y_bf16 is not the rounded y"
        _check_stats(gs.view, gb.view, tag)
        close(g2.view, R.double_layer_norm_ref(y.cpu(), ga2, be2, eps2), 1e-5, 1e-5, tag + " y2")
        # each side result alone, and y == x as the engine calls it: the same bits
        ga_ = G.flat_out((rows, D))
        ga_.view.copy_(x.cuda())
        gb2, g22 = G.flat_out((rows, D), torch.bfloat16), G.flat_out((rows, D))
        ops.layer_norm_ex(ga_.view, gad, bed, eps, y=ga_.view, y_bf16=gb2.view)
        ops.layer_norm_ex(gx.view, gad, bed, eps, ln2=(ga2d, be2d, eps2), y2=g22.view)
        torch.cuda.synchronize()
        ga_.check(tag + " in place")
        gb2.check(tag + " y_bf16 alone")
        g22.check(tag + " y2 alone")
        assert G.same_bits(ga_.view.clone(), y) and G.same_bits(gb2.view.clone(), gb.view.clone()) and G.same_bits(g22.view.clone(), g2.view.clone()), tag


@pytest.mark.parametrize("D", [8, 512, 520, 2048])
def test_row_stats_bf16(D):
    """row_stats_bf16_kernel (one wave per row, 512 columns per pass: one partial pass, one pass, one and a bit, four) on the bf16
    copy a LayerNorm left, against fp64 and against the LayerNorm's own statistics (both within the bound: at most twice apart)"""
    rows = 5
    x = rnd(rows, D, seed=D) * 1.5 + 0.3
    ga, be = rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1)
    gb, gs = G.flat_out((rows, D), torch.bfloat16), G.flat_out((rows, 4, 2))
    ops.layer_norm_ex(dev(x), dev(ga), dev(be), 1e-5, y_bf16=gb.view, y_stats=gs.view)
    gr = G.flat_out((rows, 4, 2))
    g_in = G.flat_in(gb.view.cpu())
    ops.row_stats_bf16(g_in.view, stats=gr.view)
    torch.cuda.synchronize()
    gr.check("row_stats D=%d" % D)
    assert not bool(gr.untouched().any())
    b1, b2 = _check_stats(gr.view, g_in.view, "row_stats_bf16 D=%d" % D)
    _check_stats(gs.view, gb.view, "layer_norm_ex stats D=%d" % D)
    d = (gr.view.cpu().double() - gs.view.cpu().double()).abs()
    assert bool((d[:, 0, 0] <= 2 * b1).all()) and bool((d[:, 0, 1] <= 2 * b2).all())


@pytest.mark.parametrize("S,D", [(37, 260), (1, 4), (300, 512)])
def test_rows_to_bf16(S, D):
    """rows_to_bf16_kernel on a row-strided input: torch's conversion bit for bit (round to nearest even)"""
    x = rnd(S, D, seed=S) * 3.0
    x.view(-1)[::7] *= 1e-3
    gx, go = G.strided_in(x, ld=D + 12), G.flat_out((S, D), torch.bfloat16)
    assert gx.ld != D
    ops.rows_to_bf16(gx.view, out=go.view)
    dense = ops.rows_to_bf16(dev(x))
    torch.cuda.synchronize()
    go.check("rows_to_bf16")
    assert G.same_bits(go.view.clone(), x.to(torch.bfloat16).cuda()) and G.same_bits(dense, go.view.clone())
