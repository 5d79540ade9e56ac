"""ABI kernels on row-strided, guarded operands (include/m3asr.h "Row strides").

Every strided case asserts three things: (i) parity with the fp64 reference the dense test of the same operator uses, at
that test's bound; (ii) the result is BIT-IDENTICAL to the same call on dense copies of the same data (a stride must never
change the arithmetic); (iii) the guard around every output still holds its fill pattern, while the guard around every
input holds NaN (tests/guarded.py).  Each rejection test passes a stride that the entry point refuses with M3_REQUIRE on
the host, before any launch (csrc/api.hip).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded as G
from m3asr import ops, _lib
from m3asr._lib import M3Error
from m3asr.plan import fold_layernorm
from oracle import encoder_ref as ref
from stream_kernels_ref import attention_ref as _attention_ref


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r16(t):
    return t.float().to(torch.bfloat16).double()


def close(got, want, rtol, atol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    print("%s max abs err %.3e (max |ref| %.3e, bound %.1e / %.1e)" % (what, float(err.max()), float(want.abs().max()), rtol, atol))
    assert bool((err <= bound).all()), "%s max abs err %.3e (max |ref| %.3e), worst excess %.3e" % (
        what, float(err.max()), float(want.abs().max()), float((err - bound).max()))


def dev(t):
    return t.cuda().contiguous()


# ================================================================================================ m3_linear
# Kernel families and their row thresholds, read from the dispatch code:
#   gemm_plan.hip plan_gemm, TiledF32 / TiledBf16: M >= 384 and cdiv(M, 64) * cdiv(n_out, 64) >= 160 and
#     K % 64 == 0 (fp32) / K % 128 == 0 (bf16 weights), no concat, no affine LayerNorm  -> the LDS-tiled kernels
#     (64-row tiles; 128-row tiles on long batches), else the K-split "skinny" kernels (16 * MT-row tiles, 16 columns);
#   gemm_plan.hip plan_gemm, DmaBf16: M >= 4096, bf16 a, bf16 w, K % 64 == 0, lda % 8 == 0 -> the LDS-DMA kernel (128-row tiles);
#   gemm_plan.hip plan_gemm, SplitKF32: fp32, K >= 4096, K % 64 == 0, N % 4 == 0, ldy % 4 == 0, plain epilogue,
#     <= 160 tiles of 64 x 64 -> split-K kernel + reduce (m3_linear_ws only).
def _linear_case(M, N, K, *, wdt=torch.float32, a16=False, act=_lib.ACT_NONE, resid=None, masks=None, ln=None, concat=False,
                 copy=False, stats=False, y16=False, alpha=1.0, tol=3e-5, ldy=None, ldr=None, what=""):
    """One m3_linear call with every strided operand placed by the helper, against fp64 and against the dense call.
    resid: None / "own" (own buffer, ldr != ldy) / "inplace" (y == resid on one strided view);  masks: None / "in" / "out";
    ln: None / "folded" / "affine";  concat: a2 with lda2 != lda (K split in halves)."""
    glu = act == _lib.ACT_GLU
    n_out = N // 2 if glu else N
    w16 = wdt == torch.bfloat16
    a = rnd(M, K, seed=1)
    if a16:
        a = a.to(torch.bfloat16)
    w, b = rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    res = rnd(M, n_out, seed=4) if resid else None
    T = max(1, (M + 2) // 3)                                  # three "utterances" (the last one may be cut by M)
    Bn = -(-M // T)
    lens = torch.tensor([T, max(1, T // 2), 1][:Bn] + [T] * max(0, Bn - 3), dtype=torch.int32)
    pad = (torch.arange(M) % T >= lens.repeat_interleave(T)[:M]).view(M, 1)
    kw = dict(act=act, alpha=alpha)
    ad = a.double() if not w16 else r16(a)                    # bf16 weights: A is rounded to bf16 at the MFMA input
    wd = w.double() if not w16 else r16(w)
    w_dev, b_dev = (w.to(torch.bfloat16) if w16 else w), b
    a2 = None
    if ln == "folded":
        ga, be = rnd(K, seed=5) * 0.2 + 1.0, rnd(K, seed=6, scale=0.1)
        f = fold_layernorm(w, b, ga, be)
        wf = f["ln.weight"].to(torch.bfloat16) if w16 else f["ln.weight"]
        wsum = wf.double().sum(1).float() if w16 else f["ln.wsum"]
        w_dev, b_dev = wf, f["ln.bias"]
        eps = 1e-12
        x64 = a.double()
        mu, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
        z = (ad @ wf.double().t() - mu * wsum.double()) / torch.sqrt(var + eps) + f["ln.bias"].double()
        if masks == "in":
            z = torch.where(pad, (f["ln.bias"].double() - f["ln.wbeta"].double()).expand_as(z), z)   # masked_fill(0) after the LayerNorm
        kw["ln_folded"] = (dev(wsum), dev(f["ln.wbeta"]) if masks == "in" else None, eps)
        if a16:                                               # LDS-DMA kernel: the producer's per-tile row statistics
            st = torch.zeros(M, K // 128, 2)
            for q in range(K // 128):
                blk = x64[:, 128 * q:128 * (q + 1)]
                st[:, q, 0], st[:, q, 1] = blk.sum(1).float(), (blk * blk).sum(1).float()
            kw["ln_stats"] = dev(st)
    else:
        A = ad
        if ln == "affine":
            ga, be = rnd(K, seed=5) * 0.2 + 1.0, rnd(K, seed=6, scale=0.1)
            A = F.layer_norm(A, (K,), ga.double(), be.double(), 1e-5)
            kw["ln"] = (dev(ga), dev(be), 1e-5)
        if masks == "in":
            A = A.masked_fill(pad, 0.0)
        z = A @ wd.t() + b.double()
    if glu:
        z = z[:, :n_out] * torch.sigmoid(z[:, n_out:])
    z = {_lib.ACT_RELU: F.relu, _lib.ACT_SILU: F.silu}.get(act, lambda t: t)(z)
    if masks == "out":
        z = z.masked_fill(pad, 0.0)
    want = alpha * z + (res.double() if resid else 0.0)
    if masks:
        kw.update(lens=dev(lens), rows_per_batch=T, mask_in=masks == "in", mask_out=masks == "out")

    # ---- strided, guarded placement of every operand the ABI takes with a leading dimension
    ydt = torch.bfloat16 if y16 else torch.float32
    if concat:
        k1 = K // 2
        ga_ = G.strided_in(a[:, :k1].contiguous())
        ga2 = G.strided_in(a[:, k1:].contiguous(), ld=(K - k1) + 24)           # lda2 != lda
        assert ga2.ld != ga_.ld
        a_s, a2_s, a_d, a2_d = ga_.view, ga2.view, dev(a[:, :k1]), dev(a[:, k1:])
    else:
        ga_ = G.strided_in(a)
        a_s, a2_s, a_d, a2_d = ga_.view, None, dev(a), None
    gy = G.strided_out(M, n_out, ydt, ld=ldy)
    s_kw, d_kw = dict(kw), dict(kw)
    if resid == "own":
        gr = G.strided_in(res, ld=ldr if ldr is not None else n_out + 12)
        assert gr.ld != gy.ld
        s_kw["resid"], d_kw["resid"] = gr.view, dev(res)
        y_d = None
    elif resid == "inplace":
        gy.view.copy_(res.cuda())                              # the guard keeps its pattern, the view holds the residual
        s_kw["resid"] = gy.view
        y_d = dev(res)
        d_kw["resid"] = y_d
    else:
        y_d = None
    gc = gs = None
    if copy:
        gc = G.strided_out(M, n_out, torch.bfloat16, ld=n_out + 24)
        s_kw["copy_bf16"], d_kw["copy_bf16"] = gc.view, torch.zeros(M, n_out, dtype=torch.bfloat16, device="cuda")
    if stats:
        gs = G.flat_out((M, n_out // 128, 2))
        s_kw["copy_stats"], d_kw["copy_stats"] = gs.view, torch.zeros(M, n_out // 128, 2, device="cuda")
    wd_, bd_ = dev(w_dev), dev(b_dev)
    # the kernel this case is written for is the one the dispatcher picks, for the strided and for the dense call alike
    kernel = what.split("/")[0]
    assert ops.linear_kernel(a_s, wd_, bd_, a2=a2_s, out=gy.view, **s_kw) == kernel, (what, M)
    assert ops.linear_kernel(a_d, wd_, bd_, a2=a2_d, out=y_d, out_dtype=ydt, **d_kw) == kernel, (what, M)
    y_s = ops.linear(a_s, wd_, bd_, a2=a2_s, out=gy.view, **s_kw)
    y_dense = ops.linear(a_d, wd_, bd_, a2=a2_d, out=y_d, out_dtype=ydt, **d_kw)
    torch.cuda.synchronize()
    tag = "%s M=%d N=%d K=%d ldy=%d" % (what, M, N, K, gy.ld)
    gy.check(tag + " y")
    assert not bool(gy.untouched().any()), tag + ": output elements never written"
    got = G.dense(y_s)
    assert G.same_bits(got, y_dense), tag + ": strided and dense calls differ, max %.3e" % float((got.float() - y_dense.float()).abs().max())
    if y16:
        close(got.float(), want, 2 ** -8, 2 ** -8, tag)       # one bf16 rounding of the result (8 mantissa bits)
    else:
        close(got, want, tol, tol, tag)
    if copy:
        gc.check(tag + " y_copy_bf16")
        assert G.same_bits(G.dense(gc.view), got.to(torch.bfloat16)), tag + ": bf16 copy is not the rounded result"
        assert G.same_bits(G.dense(gc.view), d_kw["copy_bf16"])
    if stats:
        gs.check(tag + " y_copy_stats")
        f64 = G.dense(gc.view).float().cpu().double()
        ts = torch.stack([torch.stack([f64[:, 128 * q:128 * (q + 1)].sum(1), (f64[:, 128 * q:128 * (q + 1)] ** 2).sum(1)], -1)
                          for q in range(n_out // 128)], 1)
        close(gs.view, ts, 1e-5, 1e-4, tag + " stats")        # bound of test_linear_bf16_dma_plain_and_residual
        assert G.same_bits(gs.view, d_kw["copy_stats"])


def _tol(family, name):
    """the bound the dense test of the same kernel and epilogue holds (test_kernels_gpu.py / test_bf16_gpu.py)"""
    if "folded" in name:   # test_linear_folded_layernorm (mean 0) / test_linear_tiled_folded_layernorm / test_linear_bf16_folded_layernorm
        return {"f32_skinny": 3e-5, "f32_tiled": 2e-4, "bf16_skinny": 1e-4, "bf16_tiled": 1e-4}[family]
    if family == "f32_skinny":   # test_linear_plain / test_linear_epilogues 2e-5, test_linear_layernorm_prologue 3e-5
        return 3e-5 if name == "affine_ln" else 2e-5
    if family == "bf16_skinny":  # test_linear_bf16_plain 2e-5, test_linear_bf16_epilogues 3e-5
        return 2e-5 if name.startswith("plain") else 3e-5
    return 3e-5                  # test_linear_tiled_plain / _epilogues, test_linear_bf16_epilogues (776 rows)


# variants shared by the four register / LDS-staged families; N: 1434 = the vocabulary width, 80 / 1040: N % 64 == 16
def _variants(n_small, n_glu, affine_and_concat):
    v = [
        ("plain", dict(N=1434)),
        ("plain_n16", dict(N=n_small)),
        ("glu", dict(N=n_glu, act=_lib.ACT_GLU)),                          # both halves of W paired into one strided output
        ("resid_own_ld", dict(N=n_small, resid="own", alpha=0.5, act=_lib.ACT_SILU)),
        ("resid_inplace", dict(N=1434, resid="inplace", alpha=0.5)),
        ("mask_in", dict(N=n_small, masks="in")),
        ("mask_out_resid", dict(N=n_small, masks="out", resid="own", act=_lib.ACT_RELU)),
        ("folded_ln", dict(N=n_small, ln="folded")),
        ("folded_ln_glu_mask_in", dict(N=n_glu, ln="folded", act=_lib.ACT_GLU, masks="in")),
        ("odd_ldy_ldr", dict(N=1434, resid="own", ldy=1434 + 9, ldr=1434 + 7)),   # fp32 y / resid: any stride (element accesses)
    ]
    if affine_and_concat:
        v += [("affine_ln", dict(N=n_small, ln="affine")), ("concat2", dict(N=n_small, concat=True))]
    return v


# gemm_f32_kernel: M <= 128 -> 16-row tiles (MT = 1); one below / at / one above a tile multiple
@pytest.mark.parametrize("name,opt", _variants(80, 160, True), ids=lambda v: v if isinstance(v, str) else "")
def test_linear_f32_skinny_strided(name, opt):
    for M in (15, 16, 17, 33):
        _linear_case(M, K=512, what="gemm_f32_kernel/" + name, tol=_tol("f32_skinny", name), **opt)


# gemm_f32_tiled_kernel: 64-row tiles, 640 = 10 tiles; n_out 1040 -> 17 column tiles (170 >= 160), 1434 -> 23
@pytest.mark.parametrize("name,opt", _variants(1040, 2080, False), ids=lambda v: v if isinstance(v, str) else "")
def test_linear_f32_tiled_strided(name, opt):
    for M in (639, 640, 641):
        _linear_case(M, K=512, what="gemm_f32_tiled_kernel/" + name, tol=_tol("f32_tiled", name), **opt)


def test_linear_f32_large_m_strided():
    """long batch on the tiled kernel's 128-row tiles (4225 = 33 * 128 + 1), and the skinny kernel's 64-row tiles (MT = 4),
    which concat / affine-LayerNorm problems keep at any M (plan_gemm keeps them off the tiled kernel)"""
    _linear_case(4225, 1040, 512, what="gemm_f32_tiled_kernel/128-row tiles", resid="own", alpha=0.5)
    for M in (639, 640, 641):
        _linear_case(M, 80, 512, what="gemm_f32_kernel/MT=4 concat2", concat=True, tol=2e-5)
        _linear_case(M, 80, 512, what="gemm_f32_kernel/MT=4 affine_ln", ln="affine")


# gemm_bf16w_kernel (bf16 weights, fp32 rows): the same tiling as the fp32 skinny kernel; no concat / affine LayerNorm (rejected)
@pytest.mark.parametrize("name,opt", _variants(80, 160, False), ids=lambda v: v if isinstance(v, str) else "")
def test_linear_bf16w_skinny_strided(name, opt):
    for M in (15, 16, 17, 33):
        _linear_case(M, K=512, wdt=torch.bfloat16, what="gemm_bf16w_kernel/" + name, tol=_tol("bf16_skinny", name), **opt)


# gemm_bf16w_tiled_kernel: 64-row tiles; also bf16 rows in (lda % 8), bf16 rows out, and the bf16 copy
@pytest.mark.parametrize("name,opt", _variants(1040, 2080, False) + [
    ("a_bf16", dict(N=1040, a16=True)), ("y_bf16", dict(N=1040, y16=True, a16=True)),
    ("copy_bf16", dict(N=1040, copy=True, resid="own", alpha=0.5))], ids=lambda v: v if isinstance(v, str) else "")
def test_linear_bf16w_tiled_strided(name, opt):
    for M in (639, 640, 641):
        _linear_case(M, K=512, wdt=torch.bfloat16, what="gemm_bf16w_tiled_kernel/" + name, tol=_tol("bf16_tiled", name), **opt)


# gemm_bf16_dma_kernel: from 4096 rows, 128-row tiles: 4096 = 32 tiles, 4097 one above, 4223 = 33 * 128 - 1.  (4095 rows do
# not reach this kernel: they run the tiled one above.)
@pytest.mark.parametrize("name,opt,tol", [
    ("plain", dict(N=1434), 2e-5),
    ("plain_n16", dict(N=1040), 2e-5),
    ("copy_stats_resid", dict(N=512, copy=True, stats=True, resid="own", alpha=0.5, act=_lib.ACT_SILU), 2e-5),
    ("copy_no_stats_inplace", dict(N=1040, copy=True, resid="inplace", alpha=0.5), 2e-5),
    ("y_bf16", dict(N=1040, y16=True), 2e-5),
    ("glu_folded_ln_mask_in", dict(N=1024, act=_lib.ACT_GLU, ln="folded", masks="in"), 2e-3),   # bound of test_linear_bf16_dma_epilogues
    ("mask_out_resid", dict(N=512, masks="out", resid="own"), 2e-5),
], ids=lambda v: v if isinstance(v, str) else "")
def test_linear_bf16_dma_strided(name, opt, tol):
    for M in (4096, 4097, 4223):
        _linear_case(M, K=512, wdt=torch.bfloat16, a16=True, what="gemm_bf16_dma_kernel/" + name, tol=tol, **opt)


@pytest.mark.parametrize("M,N,K,act", [(50, 512, 9728, _lib.ACT_NONE), (7, 64, 4096, _lib.ACT_SILU), (130, 100, 8192, _lib.ACT_RELU),
                                         (63, 1040, 4096, _lib.ACT_NONE), (65, 80, 4096, _lib.ACT_NONE)])
def test_linear_split_k_strided(M, N, K, act):
    """m3_linear_ws: strided a / y, the workspace guarded on both sides with exactly m3_linear_workspace_size bytes handed in."""
    a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    ga, gy = G.strided_in(a), G.strided_out(M, N)
    d = _lib.LinearDesc()
    d.a, d.lda, d.w, d.M, d.N, d.K, d.ldy = 1, ga.ld, 1, M, N, K, gy.ld
    need = _lib.load().m3_linear_workspace_size(d)
    assert need > 0, "not a split-K problem"
    assert _lib.load().m3_linear_kernel(d, 1) == b"gemm_f32_splitk_kernel"
    ws = G.flat_out((need,), torch.uint8)
    ops.linear(ga.view, dev(w), dev(b), act=act, alpha=0.5, split_k=True, out=gy.view, workspace=ws.view)
    y_d = ops.linear(dev(a), dev(w), dev(b), act=act, alpha=0.5, split_k=True)
    torch.cuda.synchronize()
    gy.check("split-K y")
    ws.check("split-K workspace")
    assert not bool(gy.untouched().any())
    want = F.linear(a.double(), w.double(), b.double())
    want = {_lib.ACT_NONE: want, _lib.ACT_RELU: F.relu(want), _lib.ACT_SILU: F.silu(want)}[act] * 0.5
    close(gy.view, want, 3e-5, 3e-5, "split-K M=%d N=%d K=%d" % (M, N, K))
    assert G.same_bits(G.dense(gy.view), y_d)


def _desc_call(**kw):
    """m3_linear on a descriptor whose strides are wrong: must fail on the host (pointers are never dereferenced there;
    they are real, valid buffers all the same)."""
    M, N, K = 8, 16, 32
    a, w, y = torch.zeros(M + 2, 64, device="cuda"), torch.zeros(N, K, device="cuda"), torch.zeros(M + 2, 64, device="cuda")
    yb = torch.zeros(M + 2, 64, dtype=torch.bfloat16, device="cuda")
    d = _lib.LinearDesc()
    d.a, d.lda, d.w, d.y, d.ldy, d.M, d.N, d.K = a.data_ptr(), 64, w.data_ptr(), y.data_ptr(), 64, M, N, K
    d.alpha = 1.0
    for k, v in kw.items():
        if k == "resid":
            d.resid = y.data_ptr()
        elif k == "a2":
            d.a2, d.k1 = a.data_ptr(), 16
        elif k == "copy":
            d.y_copy_bf16, d.weight_dtype = yb.data_ptr(), _lib.BF16
        elif k == "ybf16":
            d.y, d.y_dtype, d.weight_dtype = yb.data_ptr(), _lib.BF16, _lib.BF16
        elif k == "abf16":
            d.a, d.a_dtype, d.weight_dtype = yb.data_ptr(), _lib.BF16, _lib.BF16
        else:
            setattr(d, k, v)
    return _lib.load().m3_linear(d, None)


@pytest.mark.parametrize("kw", [dict(lda=31), dict(lda=28), dict(lda=66), dict(ldy=15), dict(resid=1, ldr=15), dict(a2=1, lda=16, lda2=12),
                                dict(a2=1, lda=16, lda2=18), dict(copy=1, ld_copy=18), dict(copy=1, ld_copy=12), dict(ybf16=1, ldy=18),
                                dict(abf16=1, lda=36)], ids=str)
def test_linear_rejects_bad_strides(kw):
    """api.hip linear_params: lda / lda2 below the row width or not a multiple of 4 (8 for bf16 a); ldy / ldr / ld_copy below
    n_out; ld_copy / a bf16 ldy not a multiple of 4.  The checks run before launch_gemm_f32 is entered."""
    assert _desc_call() == 0                              # the same descriptor with legal strides is accepted
    assert _desc_call(**kw) != 0
    assert "ld" in _lib.last_error()
    torch.cuda.synchronize()


# ================================================================================================ attention
ATT_SHAPES = [(1, 50, 8, 64, [50]), (2, 50, 8, 64, [50, 36]), (2, 37, 4, 128, [37, 5]), (3, 9, 2, 16, [9, 6, 1]), (1, 124, 8, 64, [124]),
              (16, 124, 8, 64, [124, 12, 99, 124, 77, 64, 65, 1, 124, 33, 120, 124, 50, 63, 17, 101]),
              (12, 70, 4, 128, [70, 66, 3, 64, 65, 70, 1, 20, 70, 70, 48, 49]),
              # more than two key tiles per wave (the dense tests stop at T = 124); 1524 = T' of the longest profile
              (1, 130, 8, 64, [130]), (2, 130, 8, 64, [1, 129]), (1, 257, 8, 64, [257]), (3, 257, 4, 128, [256, 257, 1]),
              (1, 1524, 8, 64, [1524]), (2, 1524, 8, 64, [1, 1523]),
              # one utterance per call at T = its length, so that NaN rows follow the last valid key of EVERY ragged length directly
              # (inside a batch the rows behind a short utterance are the next one's, or finite padding)
              (1, 1, 2, 16, [1]), (1, 5, 4, 128, [5]), (1, 36, 8, 64, [36]), (1, 65, 8, 64, [65]), (1, 129, 8, 64, [129]),
              (1, 256, 4, 128, [256]), (1, 1523, 8, 64, [1523])]


@pytest.mark.parametrize("B,T,H,dk,lens", ATT_SHAPES)
@pytest.mark.parametrize("chunk,left", [(0, -1), (16, 2)])
def test_relpos_attention_strided(B, T, H, dk, lens, chunk, left):
    """m3_relpos_attention / _chunk with qkv as a view (ldq = 3 D + 4), p (ldp = D + 4) and out (ldo = D + 4).  NaN guard rows follow the last utterance's block and the last row of p directly (and precede the first):
    a key or position index clamped one row too far reads NaN.  (Frames t >= len[b] INSIDE a block must hold finite values by
    the kernel's contract, attention.hip: masked keys of a partial tile are multiplied by a zero probability.  The B = 1 cases at
    T = len put the NaN rows directly behind the last key of every ragged length.)
    Bound: 3e-5 / 3e-5 as test_relpos_attention.  For T >= 130 it is the larger of that and 4 x the error of the same formula
    evaluated in fp32 on the CPU against fp64 (fp32 accumulation over T keys is the kernel's arithmetic too; factor 4 for the
    different summation order) -- measured on the CPU reference: T = 1524: 4 x 1.0e-6, i.e. 3e-5 holds."""
    D = H * dk
    qkv, p = rnd(B * T, 3 * D, seed=1), rnd(T, D, seed=2)
    u, v = rnd(H, dk, seed=3, scale=0.3), rnd(H, dk, seed=4, scale=0.3)
    L = torch.tensor(lens, dtype=torch.int32)
    want = _attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left)
    tol = 3e-5
    if T >= 130:
        e32 = float((_attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left, dtype=torch.float32).double() - want).abs().max())
        tol = max(tol, 4 * e32)
        print("T=%d: fp32 CPU reference error %.3e -> bound %.3e" % (T, e32, tol))
    gq, gp, go = G.strided_in(qkv, ld=3 * D + 4), G.strided_in(p, ld=D + 4), G.strided_out(B * T, D, ld=D + 4)
    args = (dev(u), dev(v), dev(L), B, T, H, dk)
    ops.relpos_attention(gq.view, gp.view, *args, chunk=chunk, left_chunks=left, out=go.view)
    out_d = ops.relpos_attention(dev(qkv), dev(p), *args, chunk=chunk, left_chunks=left)
    torch.cuda.synchronize()
    go.check("attention out")
    assert not bool(go.untouched().any())
    got = G.dense(go.view)
    assert G.same_bits(got, out_d), "strided and dense calls differ: %.3e" % float((got - out_d).abs().max())
    close(got, want, tol, tol, "attention B=%d T=%d H=%d dk=%d chunk=%d" % (B, T, H, dk, chunk))


@pytest.mark.parametrize("B,T,H,dk,lens", [(1, 50, 8, 64, [50]), (2, 36, 8, 64, [36, 20]), (1, 124, 8, 64, [124]), (1, 128, 8, 64, [128]),
                                           (16, 124, 8, 64, [124, 12, 99, 124, 77, 64, 65, 1, 124, 33, 120, 124, 50, 63, 17, 101]),
                                           (12, 70, 4, 128, [70, 66, 3, 64, 65, 70, 1, 20, 70, 70, 48, 49]), (3, 17, 4, 128, [17, 16, 15]),
                                           (2, 128, 4, 128, [1, 128])])
@pytest.mark.parametrize("chunk,left", [(0, -1), (16, 2)])
def test_relpos_attention_bf16_strided(B, T, H, dk, lens, chunk, left):
    """m3_relpos_attention_bf16: qkv (ldq = 3 D + 8), p (ldp = D + 4), out (ldo = D + 8) as views; bound of
    test_relpos_attention_bf16 (1.2e-2: bf16 probabilities and bf16 output) on the valid rows."""
    D = H * dk
    qkv, p = rnd(B * T, 3 * D, seed=1).to(torch.bfloat16), rnd(T, D, seed=2)
    u, v = rnd(H, dk, seed=3, scale=0.3), rnd(H, dk, seed=4, scale=0.3)
    L = torch.tensor(lens, dtype=torch.int32)
    want = _attention_ref(qkv.float(), p.to(torch.bfloat16).float(), u, v, L, B, T, H, dk, chunk, left, round_q16=True)
    gq, gp, go = G.strided_in(qkv, ld=3 * D + 8), G.strided_in(p, ld=D + 4), G.strided_out(B * T, D, torch.bfloat16, ld=D + 8)
    args = (dev(u), dev(v), dev(L), B, T, H, dk)
    ops.relpos_attention_bf16(gq.view, gp.view, *args, chunk=chunk, left_chunks=left, out=go.view)
    out_d = ops.relpos_attention_bf16(dev(qkv), dev(p), *args, chunk=chunk, left_chunks=left)
    torch.cuda.synchronize()
    go.check("attention (bf16) out")
    got = G.dense(go.view)
    valid = (torch.arange(T).view(1, -1) < L.view(-1, 1)).reshape(-1)
    assert G.same_bits(got[valid.cuda()], out_d[valid.cuda()])
    assert bool(torch.isfinite(got.float()[valid.cuda()]).all())
    close(got.float().cpu()[valid], want[valid], 1.2e-2, 1.2e-2, "attention bf16 B=%d T=%d chunk=%d" % (B, T, chunk))


@pytest.mark.parametrize("which,ldq,ldp,ldo", [("f32", 3 * 128 + 2, 128, 128), ("f32", 3 * 128, 130, 128), ("f32", 3 * 128 - 4, 128, 128),
                                                ("f32", 3 * 128, 124, 128), ("f32", 3 * 128, 128, 127), ("chunk", 3 * 128 + 2, 128, 128),
                                                ("chunk", 3 * 128, 128, 127), ("bf16", 3 * 128 + 4, 128, 128), ("bf16", 3 * 128, 128, 130),
                                                ("bf16", 3 * 128, 128, 124), ("bf16", 3 * 128, 126, 128)])
def test_relpos_attention_rejects_bad_strides(which, ldq, ldp, ldo):
    """launch_relpos_attention*: ldq / ldp multiples of 4 (8 for bf16 qkv), bf16 ldo a multiple of 4; api.hip: ldq >= 3 D,
    ldp >= D, ldo >= D.  All checked on the host before the launch; the buffers passed are large enough for any of them."""
    B, T, H, dk = 2, 8, 2, 64
    big = torch.zeros(64, 1024, device="cuda")
    big16 = torch.zeros(64, 1024, dtype=torch.bfloat16, device="cuda")
    u = torch.zeros(H, dk, device="cuda")
    L = torch.full((B,), T, dtype=torch.int32, device="cuda")
    lib, P = _lib.load(), lambda t: t.data_ptr()
    if which == "f32":
        rc = lib.m3_relpos_attention(P(big), ldq, P(big), ldp, P(u), P(u), P(L), B, T, H, dk, 0.125, P(big), ldo, None)
    elif which == "chunk":
        rc = lib.m3_relpos_attention_chunk(P(big), ldq, P(big), ldp, P(u), P(u), P(L), B, T, H, dk, 0.125, 4, 1, P(big), ldo, None)
    else:
        rc = lib.m3_relpos_attention_bf16(P(big16), ldq, P(big), ldp, P(u), P(u), P(L), B, T, H, dk, 0.125, 0, -1, P(big16), ldo, None)
    assert rc != 0 and "attention" in _lib.last_error()
    torch.cuda.synchronize()


# ================================================================================================ router / gate / quantise
@pytest.mark.parametrize("S,E,De,D", [(50, 32, 512, 512), (1, 64, 512, 512), (17, 16, 64, 128), (1090, 32, 512, 512), (4480, 64, 512, 512),
                                      (333, 48, 256, 1024), (50, 8, 512, 512), (15, 32, 512, 512), (16, 32, 512, 512)])
def test_moe_router_strided(S, E, De, D):
    """m3_moe_router with all four strides different from their widths (ld_logits odd: the logits are element stores);
    shapes and bounds of test_moe_router."""
    emb, x = rnd(S, De, seed=1), rnd(S, D, seed=2) * 1.7 + 0.4
    wr, b = rnd(E, De + D, seed=3, scale=0.5), rnd(E, seed=4)
    ga, be = rnd(D, seed=5, scale=0.3) + 1.0, rnd(D, seed=6, scale=0.2)
    eps = 1e-12
    want_xn = F.layer_norm(x.double(), (D,), ga.double(), be.double(), eps)
    want = torch.cat([emb.double(), want_xn], -1) @ wr.double().t() + b.double()
    ge, gx = G.strided_in(emb), G.strided_in(x, ld=D + 20)
    gl, gn = G.strided_out(S, E, ld=E + 9), G.strided_out(S, D, ld=D + 12)
    assert len({ge.ld - De, gx.ld - D, gl.ld - E, gn.ld - D}) == 4
    ln = (dev(ga), dev(be), eps)
    ops.moe_router(ge.view, gx.view, dev(wr), ln, bias=dev(b), out=gl.view, xn_out=gn.view)
    y_d, xn_d = ops.moe_router(dev(emb), dev(x), dev(wr), ln, bias=dev(b))
    torch.cuda.synchronize()
    gl.check("router logits")
    gn.check("router xn")
    assert not bool(gl.untouched().any()) and not bool(gn.untouched().any())
    assert G.same_bits(G.dense(gl.view), y_d) and G.same_bits(G.dense(gn.view), xn_d)
    close(gn.view, want_xn, 2e-5, 2e-5, "router xn S=%d" % S)
    close(gl.view, want, 2e-5, 2e-4, "router logits S=%d" % S)
    # xn = NULL: only the logits are written
    gl2 = G.strided_out(S, E, ld=E + 9)
    ops.moe_router(ge.view, gx.view, dev(wr), ln, bias=dev(b), want_xn=False, out=gl2.view)
    gl2.check("router logits (no xn)")
    assert G.same_bits(G.dense(gl2.view), y_d)


@pytest.mark.parametrize("bad", ["ld_embed_short", "ld_embed_odd", "ldx_short", "ldx_odd", "ld_xn_short", "ld_xn_odd", "ld_logits_short"])
def test_moe_router_rejects_bad_strides(bad):
    S, E, De, D = 8, 16, 64, 64
    big, big_e, o_xn, o_l = [torch.zeros(32, 256, device="cuda") for _ in range(4)]
    w, g = torch.zeros(E, De + D, device="cuda"), torch.ones(D, device="cuda")
    ld = dict(ld_embed=De + 4, ldx=D + 4, ld_xn=D + 4, ld_logits=E + 1)
    name, kind = bad.rsplit("_", 1)
    width = dict(ld_embed=De, ldx=D, ld_xn=D, ld_logits=E)[name]
    lib, P = _lib.load(), lambda t: t.data_ptr()
    call = lambda l: lib.m3_moe_router(P(big_e), l["ld_embed"], De, P(big), l["ldx"], D, P(w), None, P(g), P(g), 1e-5, P(o_xn), l["ld_xn"],
                                       P(o_l), l["ld_logits"], S, E, None)
    assert call(ld) == 0
    ld[name] = width - 4 if kind == "short" else width + 2
    assert call(ld) != 0 and "moe_router" in _lib.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T,E,ld", [(1, 50, 32, 36), (3, 17, 64, 68), (2, 9, 4, 8), (2, 9, 4, 64), (1, 5, 4, 9)])
def test_softmax_top1_strided(B, T, E, ld):
    """m3_softmax_top1 on a logits view with ld = E + 4, ld = 64 for E = 4, and an odd ld (element loads); ties and masked rows
    as in test_softmax_top1; idx exact, value at its bound, both bit-identical to the dense call, outputs guarded."""
    logits = rnd(B, T, E, seed=B * T, scale=4.0)
    logits[0, 0, :] = 0.0
    logits[0, 1, 1] = logits[0, 1, 2] = 9.0
    lens = torch.tensor([T] + [max(1, T - 3 * i) for i in range(1, B)], dtype=torch.int32)
    v_ref, i_ref = ref.softmax_topk(logits, lens.long())
    gl = G.strided_in(logits.view(B * T, E), ld=ld)
    lens_d = dev(lens)
    val, idx = ops.softmax_top1(gl.view, lens_d, T)
    val_d, idx_d = ops.softmax_top1(dev(logits), lens_d, T)
    assert torch.equal(idx.cpu().view(B, T, 1), i_ref) and torch.equal(idx, idx_d)
    assert G.same_bits(val, val_d)
    close(val.view(B, T, 1), v_ref, 1e-5, 1e-7, "softmax_top1 value")
    # the dense outputs, guarded: called through the ABI on flat-guarded buffers
    gi, gv = G.flat_out((B * T,), torch.int32), G.flat_out((B * T,))
    rc = _lib.load().m3_softmax_top1(gl.view.data_ptr(), gl.ld, lens_d.data_ptr(), T, B * T, E, gi.view.data_ptr(), gv.view.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    gi.check("softmax_top1 idx")
    gv.check("softmax_top1 value")
    assert torch.equal(gi.view, idx_d) and G.same_bits(gv.view, val_d)


def test_softmax_top1_rejects_short_stride():
    x = torch.zeros(16, 64, device="cuda")
    out_i, out_v = torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros(16, device="cuda")
    lib = _lib.load()
    assert lib.m3_softmax_top1(x.data_ptr(), 64, None, 0, 16, 32, out_i.data_ptr(), out_v.data_ptr(), None) == 0
    assert lib.m3_softmax_top1(x.data_ptr(), 31, None, 0, 16, 32, out_i.data_ptr(), out_v.data_ptr(), None) != 0
    assert "softmax_topk" in _lib.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [1, 3, 4, 5, 3000])
def test_quantize_rows_e4m3_strided(S):
    """m3_quantize_rows_e4m3 with ldx = 516: bit-exact against the dense call; at S = 3000 (the data of
    test_quantize_rows_e4m3_matches_torch_conversion) also against the torch conversion, with that test's assertions;
    xq / scale (dense in the ABI) guarded."""
    D = 512
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3000, D, generator=g) * torch.logspace(-3, 3, 3000).view(-1, 1))
    x[17] = 0.0
    x = x[:S].contiguous() if S < 3000 else x
    gx = G.strided_in(x, ld=516)
    xq, sc = ops.quantize_rows_e4m3(gx.view)
    xq_d, sc_d = ops.quantize_rows_e4m3(dev(x))
    assert torch.equal(xq, xq_d) and G.same_bits(sc, sc_d)
    amax = x.abs().amax(1).clamp_min(1e-30)
    assert torch.equal(sc.cpu(), amax * (1.0 / 448.0))
    if S == 3000:
        want = (x * (448.0 / amax).view(-1, 1)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        neq = (xq.cpu() != want)
        print("quantize_rows_e4m3 (ldx = 516): %d of %d bytes differ from torch's conversion" % (int(neq.sum()), neq.numel()))
        assert int(neq.sum()) <= neq.numel() // 20000
        assert bool((xq.cpu()[17] == 0).all())
    gq, gs = G.flat_out((S, D), torch.uint8), G.flat_out((S,))
    rc = _lib.load().m3_quantize_rows_e4m3(gx.view.data_ptr(), gx.ld, S, D, gq.view.data_ptr(), gs.view.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    gq.check("xq")
    gs.check("scale")
    assert torch.equal(gq.view, xq_d) and G.same_bits(gs.view, sc_d)


@pytest.mark.parametrize("ldx", [508, 514])
def test_quantize_rows_e4m3_rejects_bad_stride(ldx):
    x, q, s = torch.zeros(8, 1024, device="cuda"), torch.zeros(8, 512, dtype=torch.uint8, device="cuda"), torch.zeros(8, device="cuda")
    lib = _lib.load()
    assert lib.m3_quantize_rows_e4m3(x.data_ptr(), 1024, 8, 512, q.data_ptr(), s.data_ptr(), None) == 0
    assert lib.m3_quantize_rows_e4m3(x.data_ptr(), ldx, 8, 512, q.data_ptr(), s.data_ptr(), None) != 0
    assert "quantize_rows_e4m3" in _lib.last_error()
    torch.cuda.synchronize()


# ================================================================================================ base pointers, aliasing
def test_linear_rejects_misaligned_pointers_and_mixed_inplace_strides():
    """m3_linear: a / y / resid 4 bytes off a 16-byte boundary (their strides are multiples of 4, so the tiled kernels would
    use 16-byte accesses), and y == resid with ldr != ldy; refused by linear_pointers on the host before the launch."""
    M, N, K = 8, 16, 32
    a, w, y = torch.zeros(M + 2, 64, device="cuda"), torch.zeros(N, K, device="cuda"), torch.zeros(M + 2, 64, device="cuda")

    def call(a_off=0, y_off=0, resid=None, ldr=64):
        d = _lib.LinearDesc()
        d.a, d.lda, d.w, d.y, d.ldy, d.M, d.N, d.K = a.data_ptr() + a_off, 64, w.data_ptr(), y.data_ptr() + y_off, 64, M, N, K
        d.alpha = 1.0
        if resid is not None:
            d.resid, d.ldr = resid, ldr
        return _lib.load().m3_linear(d, None)

    assert call() == 0 and call(resid=y.data_ptr(), ldr=64) == 0
    assert call(a_off=4) != 0 and "aligned" in _lib.last_error()
    assert call(y_off=4) != 0 and "aligned" in _lib.last_error()
    assert call(resid=a.data_ptr() + 4) != 0 and "aligned" in _lib.last_error()
    assert call(resid=y.data_ptr(), ldr=68) != 0 and "in-place" in _lib.last_error()
    torch.cuda.synchronize()


def test_row_operators_reject_misaligned_pointers():
    """attention, router and quantiser: a row operand 4 bytes off a 16-byte boundary is refused on the host"""
    lib, P = _lib.load(), lambda t: t.data_ptr()
    B, T, H, dk = 2, 8, 2, 64
    big, out = torch.zeros(64, 1024, device="cuda"), torch.zeros(64, 1024, device="cuda")
    u = torch.zeros(H, dk, device="cuda")
    L = torch.full((B,), T, dtype=torch.int32, device="cuda")
    att = lambda q, p, o: lib.m3_relpos_attention(q, 384, p, 128, P(u), P(u), P(L), B, T, H, dk, 0.125, o, 128, None)
    assert att(P(big), P(big), P(out)) == 0
    for args in ((P(big) + 4, P(big), P(out)), (P(big), P(big) + 4, P(out)), (P(big), P(big), P(out) + 4)):
        assert att(*args) != 0 and "aligned" in _lib.last_error()
    S, E, De, D = 8, 16, 64, 64
    w, g = torch.zeros(E, De + D, device="cuda"), torch.ones(D, device="cuda")
    xn, lg = torch.zeros(32, 256, device="cuda"), torch.zeros(32, 256, device="cuda")
    rt = lambda e, x, n: lib.m3_moe_router(e, 68, De, x, 68, D, P(w), None, P(g), P(g), 1e-5, n, 68, P(lg), 17, S, E, None)
    assert rt(P(big), P(out), P(xn)) == 0
    for args in ((P(big) + 4, P(out), P(xn)), (P(big), P(out) + 4, P(xn)), (P(big), P(out), P(xn) + 4)):
        assert rt(*args) != 0 and "aligned" in _lib.last_error()
    q, sc = torch.zeros(8, 512, dtype=torch.uint8, device="cuda"), torch.zeros(8, device="cuda")
    assert lib.m3_quantize_rows_e4m3(P(big), 1024, 8, 512, P(q), P(sc), None) == 0
    assert lib.m3_quantize_rows_e4m3(P(big) + 4, 1024, 8, 512, P(q), P(sc), None) != 0 and "aligned" in _lib.last_error()
    torch.cuda.synchronize()
