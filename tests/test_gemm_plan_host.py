"""The dense GEMM's form is decided in one place (plan_gemm, csrc/gemm_plan.hip).  This table pins what it answers, through the
host-only entries m3_linear_kernel(desc, 0), m3_linear_kernel(desc, 1) and m3_linear_workspace_size(desc); no GPU is needed.

How the expected column was obtained: NOT from the planner.  A scratch script built the library of the commit before the
planner existed and asked it the same three questions for every row below.  That library named a kernel by sizes alone, also
for problems its launchers then refused; for those rows the script called its m3_linear with placeholder operands: the launcher
fails on the CPU with its check's own message in m3_last_error() before any HIP call (a row it accepts fails later, in HIP, with
a "<file>:<line>: ... failed: ..." message).  Such rows are recorded as rejected, with that message; their label is None, which
is what ops.linear_kernel always documented.  The message is checked too, through m3_linear.

The boundaries, each from both sides: 383 / 384 rows at N = 2048, K = 512 (M3_TILED_MIN_ROWS, 192 tiles of 64 x 64); the 160-tile
bound at N = 1024 (576 rows = 144 tiles, 640 rows = 160 tiles), plain and under GLU (N = 2048, 1024 columns out); K = 512
against K = 544 (a multiple of 32, not of 64) and 576 (of 64, not of 128); concat operands with and without the affine
LayerNorm (m3_linear has no ln_on_a2, so the affine LayerNorm next to a concat is refused: no affine-LayerNorm concat row is
reachable) and the affine LayerNorm on plain rows; bf16 `a` at 4095 / 4096 rows (M3_DMA_MIN_ROWS), with the folded LayerNorm
with and without ln_stats, below 384 rows (no kernel), fp32 `a` at 4096 rows; y_copy_stats below the LDS-DMA threshold; split-K
at K = 4096 / 4032, 160 / 176 tiles, N % 4 != 0, a residual, bf16 weights, each with and without a workspace; the model's own
B = 1 rows (M = 50).  The implicit-conv path is not in this table (its rows were left to the GPU tier when the table was
made, tests/test_kernels_gpu.py, tests/test_strided_operands_gpu.py); its host-only query, m3_conv2d_3x3s2_kernel, is pinned in
tests/test_packed_forms_host.py."""
import ctypes as C

import pytest

from m3asr import _lib

F32, BF16 = 0, 4                                   # m3_dtype (include/m3asr.h)
ACT = {None: 0, "relu": 1, "silu": 2, "glu": 3}    # m3_act

SKINNY, SKINNY16 = "gemm_f32_kernel", "gemm_bf16w_kernel"
TILED, TILED16 = "gemm_f32_tiled_kernel", "gemm_bf16w_tiled_kernel"
DMA, SPLITK = "gemm_bf16_dma_kernel", "gemm_f32_splitk_kernel"


def row(M, N, K, w="f32", a="f32", y="f32", act=None, ln=None, ln_stats=False, copy=False, copy_stats=False, resid=False, k1=0,
        mask_in=False, alpha=1.0):
    return dict(M=M, N=N, K=K, w=w, a=a, y=y, act=act, ln=ln, ln_stats=ln_stats, copy=copy, copy_stats=copy_stats, resid=resid, k1=k1,
                mask_in=mask_in, alpha=alpha)


# (row, (kernel without workspace, kernel with workspace, workspace bytes), the launcher's message for a row it refuses)
TABLE = [
    # ---- M3_TILED_MIN_ROWS: 383 / 384 rows, 192 tiles of 64 x 64 either side
    (row(383, 2048, 512), (SKINNY, SKINNY, 0), None),
    (row(384, 2048, 512), (TILED, TILED, 0), None),
    (row(383, 2048, 512, w="bf16"), (SKINNY16, SKINNY16, 0), None),
    (row(384, 2048, 512, w="bf16"), (TILED16, TILED16, 0), None),
    # ---- the 160-tile bound at N = 1024: 144 tiles, 160 tiles
    (row(576, 1024, 512), (SKINNY, SKINNY, 0), None),
    (row(640, 1024, 512), (TILED, TILED, 0), None),
    (row(576, 1024, 512, w="bf16"), (SKINNY16, SKINNY16, 0), None),
    (row(640, 1024, 512, w="bf16"), (TILED16, TILED16, 0), None),
    # ---- the same under GLU: the tiles are counted over the 1024 output columns
    (row(576, 2048, 512, act="glu", ln="folded"), (SKINNY, SKINNY, 0), None),
    (row(640, 2048, 512, act="glu", ln="folded"), (TILED, TILED, 0), None),
    (row(576, 2048, 512, w="bf16", act="glu"), (SKINNY16, SKINNY16, 0), None),
    (row(640, 2048, 512, w="bf16", act="glu"), (TILED16, TILED16, 0), None),
    # ---- K multiples the tiled kernels need: 64 in fp32, 128 in bf16
    (row(640, 1024, 544), (SKINNY, SKINNY, 0), None),
    (row(640, 1024, 576), (TILED, TILED, 0), None),
    (row(640, 1024, 544, w="bf16"), (SKINNY16, SKINNY16, 0), None),
    (row(640, 1024, 576, w="bf16"), (SKINNY16, SKINNY16, 0), None),
    (row(640, 1024, 528), (SKINNY, SKINNY, 0), None),
    (row(640, 1024, 528, w="bf16"), (None, None, 0), "gemm_bf16w: K=528 must be a multiple of 32"),
    # ---- concat operands and the affine LayerNorm stay on the skinny fp32 kernel at any size; bf16 has neither
    (row(2000, 32, 768, k1=256), (SKINNY, SKINNY, 0), None),
    (row(640, 1024, 768, k1=256), (SKINNY, SKINNY, 0), None),
    (row(640, 1024, 768, k1=256, ln="affine"), (None, None, 0), "gemm: LayerNorm needs plain A (or the A2 half of a concat)"),
    (row(640, 1024, 512, ln="affine"), (SKINNY, SKINNY, 0), None),
    (row(640, 1024, 768, k1=256, w="bf16"), (None, None, 0), "gemm_bf16w: concat operands are fp32-only (the router stays fp32)"),
    (row(640, 1024, 768, k1=256, w="bf16", ln="affine"), (None, None, 0),
     "gemm_bf16w: concat operands are fp32-only (the router stays fp32)"),
    (row(640, 1024, 512, w="bf16", ln="affine"), (None, None, 0),
     "gemm_bf16w: only the folded LayerNorm (ln_wsum) is available with bf16 weights"),
    # ---- bf16 `a`: M3_DMA_MIN_ROWS, the folded LayerNorm's row statistics, no kernel below the tiled one
    (row(4095, 512, 512, w="bf16", a="bf16"), (TILED16, TILED16, 0), None),
    (row(4096, 512, 512, w="bf16", a="bf16"), (DMA, DMA, 0), None),
    (row(4096, 1536, 512, w="bf16", a="bf16", ln="folded", ln_stats=True), (DMA, DMA, 0), None),
    (row(4096, 1536, 512, w="bf16", a="bf16", ln="folded"), (TILED16, TILED16, 0), None),
    (row(4096, 512, 512, w="bf16", a="bf16", y="bf16", copy=True, copy_stats=True, resid=True), (DMA, DMA, 0), None),
    (row(4096, 512, 512, w="bf16"), (TILED16, TILED16, 0), None),
    (row(383, 2048, 512, w="bf16", a="bf16"), (None, None, 0), "gemm_bf16w: bf16 activations are a feature of the tiled kernel"),
    (row(383, 2048, 512, w="bf16", y="bf16"), (None, None, 0), "gemm_bf16w: bf16 activations are a feature of the tiled kernel"),
    (row(2048, 512, 512, w="bf16", a="bf16", copy=True, copy_stats=True), (None, None, 0),
     "gemm_bf16w: y_copy_stats / ln_stats need the LDS-DMA kernel (M >= 4096 rows, bf16 A); this problem (M=2048) runs on another one"),
    (row(4095, 1536, 512, w="bf16", a="bf16", ln="folded", ln_stats=True), (None, None, 0),
     "gemm_bf16w: y_copy_stats / ln_stats need the LDS-DMA kernel (M >= 4096 rows, bf16 A); this problem (M=4095) runs on another one"),
    # ---- split-K: only with a workspace; K >= 4096, at most 160 tiles, N % 4 == 0, plain epilogue, fp32 weights
    (row(50, 512, 4096, act="relu"), (SKINNY, SPLITK, 16 * 50 * 512 * 4), None),
    (row(50, 512, 4032), (SKINNY, SKINNY, 0), None),
    (row(50, 512, 9728), (SKINNY, SPLITK, 38 * 50 * 512 * 4), None),
    (row(640, 1024, 4096), (TILED, SPLITK, 3 * 640 * 1024 * 4), None),
    (row(641, 1024, 4096), (TILED, TILED, 0), None),
    (row(50, 510, 4096), (SKINNY, SKINNY, 0), None),
    (row(50, 512, 4096, resid=True), (SKINNY, SKINNY, 0), None),
    (row(50, 512, 4096, w="bf16"), (SKINNY16, SKINNY16, 0), None),
    # ---- one utterance (M = 50): every block GEMM of the model
    (row(50, 1536, 512, ln="folded"), (SKINNY, SKINNY, 0), None),
    (row(50, 512, 512, resid=True), (SKINNY, SKINNY, 0), None),
    (row(50, 1024, 512, act="glu", ln="folded"), (SKINNY, SKINNY, 0), None),
    (row(50, 2048, 512, act="silu", ln="folded", mask_in=True), (SKINNY, SKINNY, 0), None),
    (row(50, 512, 2048, resid=True, alpha=0.5), (SKINNY, SKINNY, 0), None),
    (row(50, 32, 768, k1=256), (SKINNY, SKINNY, 0), None),
    (row(50, 1434, 512), (SKINNY, SKINNY, 0), None),
    (row(50, 1536, 512, w="bf16", ln="folded"), (SKINNY16, SKINNY16, 0), None),
    (row(50, 512, 512, w="bf16", resid=True), (SKINNY16, SKINNY16, 0), None),
    (row(50, 1024, 512, w="bf16", act="glu", ln="folded"), (SKINNY16, SKINNY16, 0), None),
    (row(50, 512, 2048, w="bf16", resid=True, alpha=0.5), (SKINNY16, SKINNY16, 0), None),
    (row(50, 512, 9728, w="bf16"), (SKINNY16, SKINNY16, 0), None),
]

_HOST = (C.c_char * 4096)()      # placeholder operands: 16-byte aligned, never read (m3_linear is called on refused rows only)
_PTR = (C.addressof(_HOST) + 15) // 16 * 16


def desc(r):
    d = _lib.LinearDesc()
    n_out = r["N"] // 2 if r["act"] == "glu" else r["N"]
    k1 = r["k1"] or r["K"]
    d.a, d.lda, d.w, d.y, d.ldy = _PTR, k1, _PTR, _PTR, n_out
    if r["k1"]:
        d.a2, d.lda2, d.k1 = _PTR, r["K"] - k1, k1
    d.M, d.N, d.K = r["M"], r["N"], r["K"]
    d.bias, d.ln_eps, d.act, d.alpha = _PTR, 1e-5, ACT[r["act"]], r["alpha"]
    if r["ln"] == "folded":
        d.ln_wsum, d.ln_wbeta = _PTR, _PTR
    if r["ln"] == "affine":
        d.ln_gamma, d.ln_beta = _PTR, _PTR
    if r["mask_in"]:
        d.len, d.rows_per_batch, d.mask_in = _PTR, r["M"], 1
    if r["resid"]:
        d.resid, d.ldr = _PTR + 2048, n_out
    d.weight_dtype = BF16 if r["w"] == "bf16" else F32
    d.a_dtype = BF16 if r["a"] == "bf16" else F32
    d.y_dtype = BF16 if r["y"] == "bf16" else F32
    if r["copy"]:
        d.y_copy_bf16, d.ld_copy = _PTR, n_out
    if r["copy_stats"]:
        d.y_copy_stats = _PTR
    if r["ln_stats"]:
        d.ln_stats, d.ln_stat_parts = _PTR, 4
    return d


def query(lib, r):
    d = desc(r)
    k0, k1 = lib.m3_linear_kernel(C.byref(d), 0), lib.m3_linear_kernel(C.byref(d), 1)
    return (k0.decode() if k0 else None, k1.decode() if k1 else None, lib.m3_linear_workspace_size(C.byref(d)))


def _id(r):
    on = [k if v is True else "%s=%s" % (k, v) for k, v in r.items() if k not in ("M", "N", "K") and (v is True or v not in (False, None, 0, 1.0, "f32"))]
    return "-".join(["%dx%dx%d" % (r["M"], r["N"], r["K"])] + on)


def test_table_covers_every_form():
    """what keeps the table from silently covering less: all six GemmKernel labels and refused rows are expected somewhere"""
    assert {k for _, want, _ in TABLE for k in want[:2]} == {SKINNY, SKINNY16, TILED, TILED16, DMA, SPLITK, None}
    assert len({_id(r) for r, _, _ in TABLE}) == len(TABLE)
    assert all((msg is None) == (want[0] is not None) for _, want, msg in TABLE)


@pytest.mark.parametrize("r,want,msg", TABLE, ids=[_id(r) for r, _, _ in TABLE])
def test_form_matches_the_dispatchers_it_replaced(r, want, msg):
    lib = _lib.load()
    assert query(lib, r) == want
    if msg is not None:      # refused by the plan, on the host: same text as the launcher's own check gave
        assert lib.m3_linear(C.byref(desc(r)), None) != 0
        assert _lib.last_error() == msg
