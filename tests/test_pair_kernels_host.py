"""Which pairs the paired-launch entries take, pinned on the host: m3_linear_pair_kernel(a, b, with_workspace) on both sides of
every boundary of the dual GEMM kernels, and the refusal messages of all pair entries.  No GPU is needed: the query reads sizes
only, and a refused pair fails on the CPU, in the entry's checks, before any HIP call (as tests/test_gemm_plan_host.py describes
for m3_linear), so placeholder host pointers are never dereferenced.

How the expected column was obtained: by hand from the rules in csrc/kernels.h and csrc/gemm_plan.hip, NOT from the planner.

  gemm_f32_dual_kernel is instantiated for 16-row tiles (mt = 1), NW = 4 or 8 waves and ONE load group per wave (nbuf = 1), with or
  without GLU and with or without the folded LayerNorm; the two problems must agree in NW, GLU and LayerNorm (gemm_dual_fusable).

  waves   skinny_grid: NW = 4 for K < 1024, 8 for 1024 <= K < 2048, 16 from 2048 on (no dual instantiation).
  groups  a wave's K-steps are K / 16 over NW waves; one load group holds gemm_group_steps(MT = 1, NT, NW) = 8 steps for NW = 4 and
          for NW = 8 alike (NT = 2 under GLU: still 8).  nbuf = 1 iff K / 16 <= 8 NW:
            K = 512:  32 steps <= 32  -> one group, pairs        K = 528:  33 > 32  -> two groups, refused
            K = 1024: 64 steps <= 64  -> one group, pairs        K = 1040: 65 > 64  -> two groups, refused
  rows    mt starts at 1 for M <= 128 and at 2 for 129 <= M <= 512, and is halved again while cdiv(N, 16) * cdiv(M, 16 mt) < 256
          (narrow outputs: fat tiles would idle the chip).
            N = 512:  M = 128 -> mt 1.  M = 129 -> mt 2, 32 column tiles x cdiv(129, 32) = 5 row tiles = 160 < 256 -> halved to 1: pairs.
            N = 1024: M = 128 -> mt 1.  M = 129 -> mt 2, 64 x 5 = 320 >= 256 -> stays 2: 32-row tiles, refused.
            M = 200, N = 1024: mt 2, 64 x 7 = 448 >= 256 -> 32-row tiles, refused.
  split-K needs K >= 4096 (and K % 64 == 0, few tiles, a plain epilogue): none of the K above is a split-K problem, so WITH workspaces
          every one of those pairs is refused (m3_linear_ws_pair runs gemm_f32_splitk_dual_kernel or nothing); K = 4224 / 4096
          at M = 130 / 7, N = 64 are split-K problems (66 and 64 k-steps of 64, 3 and 1 tiles) and pair only with workspaces: without
          one they plan as the skinny kernel with 16 waves (256 and 264 steps over 16 waves of 4-step groups: two groups).
"""
import ctypes as C

import pytest

from m3asr import _lib
from test_gemm_plan_host import _PTR, desc, row

DUAL, SPLITK_DUAL = "gemm_f32_dual_kernel", "gemm_f32_splitk_dual_kernel"
NO_SPLITK = "linear pair (workspaces): problem %d is no split-K problem with its workspace (it runs %s)"
SHAPE = ("linear pair: problem %d has %d-row tiles, %d waves, %d load group%s: the paired kernel takes 16-row tiles, 4 or 8 waves, one load "
         "group, plain a, no affine LayerNorm")
DIFFER = "linear pair: the problems differ in waves (%d / %d), folded LayerNorm (%d / %d) or GLU (%d / %d)"

# (first problem, second problem, label without workspaces, its refusal message, label with workspaces, its refusal message)
TABLE = [
    # ---- one load group: K = 512 / 528 (4 waves), K = 1024 / 1040 (8 waves); the odd one on either side of the pair
    (row(24, 512, 512), row(17, 48, 512), DUAL, None, None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512), row(17, 48, 528), None, SHAPE % (1, 16, 4, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 528), row(17, 48, 512), None, SHAPE % (0, 16, 4, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 256, 1024), row(40, 24, 1024), DUAL, None, None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 256, 1024), row(40, 24, 1040), None, SHAPE % (1, 16, 8, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    # ---- 16-row tiles: M = 128 / 129 at N = 512 (both pair) and at N = 1024 (129 rows take 32-row tiles); M = 200
    (row(24, 512, 512), row(128, 512, 512), DUAL, None, None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512), row(129, 512, 512), DUAL, None, None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512), row(128, 1024, 512), DUAL, None, None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512), row(129, 1024, 512), None, SHAPE % (1, 32, 4, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(200, 1024, 512), row(24, 512, 512), None, SHAPE % (0, 32, 4, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    # ---- one instantiation for both: waves, GLU, folded LayerNorm
    (row(24, 512, 512), row(24, 512, 1024), None, DIFFER % (4, 8, 0, 0, 0, 0), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512, act="glu"), row(24, 512, 512), None, DIFFER % (4, 4, 0, 0, 1, 0), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 1024, 512, act="glu"), row(34, 2048, 256, act="glu"), DUAL, None, None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512, ln="folded"), row(24, 512, 512), None, DIFFER % (4, 4, 1, 0, 0, 0), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 1024, 256, act="glu", ln="folded", mask_in=True), row(34, 2048, 512, act="glu", ln="folded", mask_in=True), DUAL, None, None,
     NO_SPLITK % (0, "gemm_f32_kernel")),
    # ---- forms the dual kernel does not have: affine LayerNorm, concat operands, bf16 weights
    (row(24, 512, 512, ln="affine"), row(24, 512, 512, ln="affine"), None, SHAPE % (0, 16, 4, 1, ""), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 32, 768, k1=256), row(24, 512, 512), None, SHAPE % (0, 16, 4, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 32, 512, k1=256), row(24, 512, 512), None, SHAPE % (0, 16, 4, 1, ""), None, NO_SPLITK % (0, "gemm_f32_kernel")),
    (row(24, 512, 512), row(24, 512, 512, w="bf16"), None,
     "linear pair: problem 1 runs gemm_bf16w_kernel: only the skinny fp32 kernel (gemm_f32_kernel) pairs", None, NO_SPLITK % (0, "gemm_f32_kernel")),
    # ---- a problem the family refuses: the plan's own reason
    (row(24, 512, 520), row(24, 512, 512), None, "gemm: K=520 must be a multiple of 16", None, "gemm: K=520 must be a multiple of 16"),
    # ---- split-K problems pair with their workspaces only (16 waves without: K >= 2048)
    (row(130, 64, 4224), row(7, 64, 4096, act="silu", alpha=0.5), None, SHAPE % (0, 16, 16, 2, "s"), SPLITK_DUAL, None),
    (row(7, 64, 4096), row(24, 512, 512), None, SHAPE % (0, 16, 16, 2, "s"), None, NO_SPLITK % (1, "gemm_f32_kernel")),
    (row(7, 64, 4096, resid=True), row(7, 64, 4096), None, SHAPE % (0, 16, 16, 2, "s"), None, NO_SPLITK % (0, "gemm_f32_kernel")),
]


def _id(ra, rb):
    from test_gemm_plan_host import _id as one
    return one(ra) + "+" + one(rb)


def _pair(ra, rb):
    """two descriptors on placeholder operands; the second one's y (and resid) apart from the first's"""
    da, db = desc(ra), desc(rb)
    db.y = _PTR + 1024
    if rb["resid"]:
        db.resid = _PTR + 3072
    return da, db


def test_table_covers_both_labels_and_refusals():
    assert {t[2] for t in TABLE} == {DUAL, None} and {t[4] for t in TABLE} == {SPLITK_DUAL, None}
    assert all((t[2] is None) != (t[3] is None) and (t[4] is None) != (t[5] is None) for t in TABLE)
    assert len({_id(t[0], t[1]) for t in TABLE}) == len(TABLE)


@pytest.mark.parametrize("ra,rb,k0,msg0,k1,msg1", TABLE, ids=[_id(t[0], t[1]) for t in TABLE])
def test_linear_pair_kernel(ra, rb, k0, msg0, k1, msg1):
    lib = _lib.load()
    for ws, want, msg in ((0, k0, msg0), (1, k1, msg1)):
        da, db = _pair(ra, rb)
        got = lib.m3_linear_pair_kernel(C.byref(da), C.byref(db), ws)
        assert (got.decode() if got else None) == want, _lib.last_error()
        if want is None:
            assert _lib.last_error() == msg
    if k0 is None:       # the launch entry refuses the same pair with the same words, on the host
        da, db = _pair(ra, rb)
        assert lib.m3_linear_pair(C.byref(da), C.byref(db), None) != 0
        assert _lib.last_error() == msg0


def test_linear_pair_refuses_overlapping_outputs():
    lib = _lib.load()
    da, db = _pair(row(24, 512, 512), row(17, 48, 512))
    db.y = da.y + 4 * (23 * 512 + 508)             # the first output's last four elements (16-byte aligned)
    assert lib.m3_linear_pair(C.byref(da), C.byref(db), None) != 0
    assert _lib.last_error() == "linear pair: the two outputs overlap"
    da, db = _pair(row(24, 512, 512), row(17, 48, 512))
    da.y = db.y + 4 * (16 * 48 + 44)               # ... and the other way round
    assert lib.m3_linear_pair(C.byref(da), C.byref(db), None) != 0
    assert _lib.last_error() == "linear pair: the two outputs overlap"


def test_linear_ws_pair_refusals():
    lib = _lib.load()
    ra, rb = row(130, 64, 4224), row(7, 64, 4096, act="silu", alpha=0.5)
    need = [lib.m3_linear_workspace_size(C.byref(desc(r))) for r in (ra, rb)]
    # by hand: 66 k-steps, 3 tiles -> min(512 / 3, 66 / 4) = 16 ranges of cdiv(66, 16) = 5 steps -> cdiv(66, 5) = 14 ranges;
    #          64 k-steps, 1 tile -> min(512, 16) = 16 ranges of 4
    assert need == [14 * 130 * 64 * 4, 16 * 7 * 64 * 4]
    big = max(need)
    ws = _PTR + 2048

    def call(ws_a, bytes_a, ws_b, bytes_b, which=3, ra=ra, rb=rb):
        da, db = _pair(ra, rb)
        assert lib.m3_linear_ws_pair(C.byref(da), ws_a, bytes_a, C.byref(db), ws_b, bytes_b, which, None) != 0
        return _lib.last_error()

    assert call(ws, big, ws, big) == "linear pair (workspaces): each problem needs its own workspace"
    assert call(ws, big, ws + need[0] - 4, big) == "linear pair (workspaces): each problem needs its own workspace"
    assert call(None, 0, ws, big) == NO_SPLITK % (0, "gemm_f32_kernel")
    assert call(ws, need[0], ws + big, need[1] - 1) == NO_SPLITK % (1, "gemm_f32_kernel")
    assert call(ws, big, ws + big, big, which=0) == "linear pair (workspaces): which=0 (1 the GEMM launch, 2 the reduce launch, 3 both)"
    assert call(ws, big, ws + big, big, which=4) == "linear pair (workspaces): which=4 (1 the GEMM launch, 2 the reduce launch, 3 both)"
    assert call(ws, big, ws + big, big, rb=row(24, 512, 512)) == NO_SPLITK % (1, "gemm_f32_kernel")
    da, db = _pair(ra, rb)
    db.y = da.y
    assert lib.m3_linear_ws_pair(C.byref(da), ws, big, C.byref(db), ws + big, big, 3, None) != 0
    assert _lib.last_error() == "linear pair (workspaces): the two outputs overlap"


def _conv2d(B, T1, F1, Cc, act, out):
    d = _lib.Conv2dDesc()
    d.inp, d.w, d.bias, d.out = _PTR, _PTR, _PTR, out
    d.B, d.T1, d.F1, d.C, d.act = B, T1, F1, Cc, act
    return d


def test_conv2d_workspace_size_and_pair_refusals():
    lib = _lib.load()
    # by hand (splitk_ranges): C = 512: K = 4608 = 72 k-steps, M = 1 * 2 * 2 = 4 rows -> 8 tiles -> min(64, 18) = 18 ranges of 4;
    # C = 576: K = 5184 = 81 k-steps, M = 3 * 4 = 12 -> 9 tiles -> min(56, 20) = 20 -> ranges of cdiv(81, 20) = 5 -> 17 ranges
    assert lib.m3_conv2d_3x3s2_workspace_size(1, 5, 5, 512, _lib.ACT_RELU) == 18 * 4 * 512 * 4
    assert lib.m3_conv2d_3x3s2_workspace_size(1, 7, 9, 576, _lib.ACT_NONE) == 17 * 12 * 576 * 4
    assert lib.m3_conv2d_3x3s2_workspace_size(1, 5, 5, 448, _lib.ACT_RELU) == 0        # K = 4032 < 4096
    assert lib.m3_conv2d_3x3s2_workspace_size(1, 5, 5, 528, _lib.ACT_RELU) == 0        # C % 64 != 0
    assert lib.m3_conv2d_3x3s2_workspace_size(1, 2, 5, 512, _lib.ACT_RELU) == 0        # shorter than the kernel
    a, b = _conv2d(1, 5, 5, 512, _lib.ACT_RELU, _PTR + 1024), _conv2d(1, 7, 9, 576, _lib.ACT_NONE, _PTR + 2048)
    big, ws = 17 * 12 * 576 * 4, _PTR + 3072

    def call(a, ws_a, bytes_a, b, ws_b, bytes_b, which=3):
        assert lib.m3_conv2d_3x3s2_ws_pair(C.byref(a), ws_a, bytes_a, C.byref(b), ws_b, bytes_b, which, None) != 0
        return _lib.last_error()

    assert call(a, ws, big, b, ws, big) == "conv2d pair: each problem needs its own workspace"
    assert call(a, ws, big, b, None, 0) == "conv2d pair: problem 1 is no split-K problem with its workspace (it runs gemm_f32_kernel)"
    assert call(a, ws, big, _conv2d(1, 5, 5, 448, 0, _PTR + 2048), ws + big, big) == \
        "conv2d pair: problem 1 is no split-K problem with its workspace (it runs gemm_f32_kernel)"
    assert call(a, ws, big, _conv2d(1, 7, 9, 576, 0, _PTR + 1024), ws + big, big) == "conv2d pair: the two outputs overlap"
    assert call(a, ws, big, _conv2d(1, 2, 9, 576, 0, _PTR + 2048), ws + big, big) == "subsample_conv2: input (2,9) smaller than the kernel"
    assert call(a, ws, big, b, ws + big, big, which=5) == "conv2d pair: which=5 (1 the GEMM launch, 2 the reduce launch, 3 both)"


def _att(B, T, H, dk, out, ldq=None, ldp=None):
    d = _lib.AttentionDesc()
    D = H * dk
    d.qkv, d.ldq, d.p, d.ldp, d.pos_u, d.pos_v, d.out, d.ldo = _PTR, ldq or 3 * D, _PTR, ldp or D, _PTR, _PTR, out, D
    d.B, d.T, d.H, d.dk, d.scale, d.chunk, d.left_chunks = B, T, H, dk, dk ** -0.5, 0, -1
    return d


def test_attention_pair_refusals():
    lib = _lib.load()

    def call(a, b):
        assert lib.m3_relpos_attention_pair(C.byref(a), C.byref(b), None) != 0
        return _lib.last_error()

    ok = _att(1, 17, 3, 64, _PTR)
    far = _PTR + 2048
    pat = ("attention pair: head widths %d / %d (64 or 128 each) or row strides ldq %d / %d, ldp %d / %d (multiples of 4) are not a paired "
           "instantiation")
    assert call(ok, _att(2, 24, 4, 32, far)) == pat % (64, 32, 576, 384, 192, 128)
    assert call(_att(1, 17, 3, 16, _PTR), ok) == pat % (16, 64, 144, 576, 48, 192)
    assert call(ok, _att(1, 4, 1, 128, far, ldq=386)) == pat % (64, 128, 576, 386, 192, 128)
    assert call(ok, _att(1, 17, 3, 64, _PTR + 4 * (16 * 192 + 188))) == "attention pair: the two outputs overlap"
    assert call(ok, _att(1, 0, 3, 64, far)) == "attention pair: empty problem 1"
    assert call(ok, _att(1, 17, 3, 64, far, ldq=100)) == "attention: ldq=100 / ldo=192 shorter than the rows (576 / 192)"
    bad = _att(1, 17, 3, 64, far)
    bad.pos_u = None
    assert call(ok, bad) == "attention pair: null qkv / p / pos_u / pos_v / out"
    bad = _att(1, 17, 3, 64, far + 4)
    assert call(ok, bad) == "attention: qkv / p / out must be 16-byte aligned"


def _dw(B, T, D, K, out, causal=False, ldz=0, sig=0, ln=True):
    d = _lib.DwconvDesc()
    d.z, d.ldz, d.gate_sigmoided, d.w_kc, d.bias, d.out = _PTR, ldz, sig, _PTR, _PTR, out
    if ln:
        d.gamma, d.beta = _PTR, _PTR
    d.left_fill = _PTR if causal else None
    d.eps, d.B, d.T, d.D, d.K = 1e-5, B, T, D, K
    return d


def test_dwconv_pair_refusals():
    lib = _lib.load()

    def call(a, b):
        assert lib.m3_dwconv_ln_silu_pair(C.byref(a), C.byref(b), None) != 0
        return _lib.last_error()

    far = _PTR + 2048
    pat = ("dwconv pair: channels %d / %d, taps %d / %d, causal %d / %d, GLU on load (ldz) %d / %d: the problems must agree in each (D %% 4 == 0, "
           "<= 4096; symmetric: K odd; GLU on load: symmetric, K <= 15, 256 <= D <= 1024, ldz >= 2 D a multiple of 4)")
    ok = _dw(1, 5, 64, 15, _PTR)
    assert call(ok, _dw(2, 9, 32, 15, far)) == pat % (64, 32, 15, 15, 0, 0, 0, 0)
    assert call(ok, _dw(2, 9, 64, 7, far)) == pat % (64, 64, 15, 7, 0, 0, 0, 0)
    assert call(ok, _dw(2, 9, 64, 15, far, causal=True)) == pat % (64, 64, 15, 15, 0, 1, 0, 0)
    assert call(_dw(1, 5, 64, 8, _PTR), _dw(2, 9, 64, 8, far)) == pat % (64, 64, 8, 8, 0, 0, 0, 0)            # even K, symmetric
    assert call(_dw(1, 5, 256, 15, _PTR, ldz=512), _dw(2, 9, 256, 15, far)) == pat % (256, 256, 15, 15, 0, 0, 512, 0)
    assert call(_dw(1, 5, 128, 15, _PTR, ldz=256), _dw(2, 9, 128, 15, far, ldz=256)) == pat % (128, 128, 15, 15, 0, 0, 256, 256)
    assert call(_dw(1, 5, 256, 15, _PTR, ldz=512, sig=1), _dw(2, 9, 256, 15, far, ldz=512)) == pat % (256, 256, 15, 15, 0, 0, 512, 512)
    assert call(ok, _dw(1, 5, 64, 15, _PTR + 4 * (5 * 64 - 4))) == "dwconv pair: the two outputs overlap"
    assert call(ok, _dw(2, 9, 64, 15, far, sig=1)) == "dwconv pair: ldz=0 (sigmoided gate columns belong to the GLU-on-load form)"
    assert call(ok, _dw(0, 9, 64, 15, far)) == "dwconv pair: empty problem 1"
    assert call(_dw(1, 5, 64, 1, _PTR, causal=True), _dw(2, 9, 64, 1, far, causal=True)) == "dwconv pair: the causal conv needs K >= 2"
    bad = _dw(2, 9, 64, 15, far)
    bad.beta = None
    assert call(ok, bad) == "dwconv pair: null z / w_kc / bias / out, or gamma without beta"
    assert call(ok, _dw(2, 9, 64, 15, far + 8)) == "dwconv pair: every operand must be 16-byte aligned"


def _c1(B, T, idim, Cc, out, act=1, lens=False):
    d = _lib.Conv1Desc()
    d.feat, d.w9c, d.bias, d.out = _PTR, _PTR, _PTR, out
    d.B, d.T, d.idim, d.C, d.act = B, T, idim, Cc, act
    if lens:
        d.feat_len, d.lens_out = _PTR, _PTR + 4000
    return d


def test_conv1_pair_refusals():
    lib = _lib.load()

    def call(a, b):
        assert lib.m3_subsample_conv1_pair(C.byref(a), C.byref(b), None) != 0
        return _lib.last_error()

    far = _PTR + 2048
    ok = _c1(1, 13, 9, 4, _PTR)                      # 6 x 4 x 4 floats = 384 bytes
    shape = "conv1 pair: the two problems do not share an input shape (B %d / %d, T %d / %d, idim %d / %d)"
    assert call(ok, _c1(1, 15, 9, 4, far)) == shape % (1, 1, 13, 15, 9, 9)
    assert call(ok, _c1(1, 13, 11, 4, far)) == shape % (1, 1, 13, 13, 9, 11)
    assert call(ok, _c1(2, 13, 9, 4, far)) == shape % (1, 2, 13, 13, 9, 9)
    assert call(ok, _c1(1, 13, 9, 4, _PTR)) == "conv1 pair: the two outputs overlap"
    assert call(ok, _c1(1, 13, 9, 4, _PTR + 368)) == "conv1 pair: the two outputs overlap"
    assert call(ok, _c1(1, 13, 9, 4, far, lens=True)) == "conv1 pair: feat_len and lens_out go together, on the first problem only"
    assert call(ok, _c1(1, 13, 9, 6, far)) == "conv1 pair: channels=6 must be a multiple of 4 (<= 1024)"
    assert call(ok, _c1(1, 13, 9, 1028, far)) == "conv1 pair: channels=1028 must be a multiple of 4 (<= 1024)"
    assert call(ok, _c1(1, 13, 9, 4, far, act=2)) == "conv1 pair: act 2 (none / relu)"
    assert call(_c1(1, 2, 9, 4, _PTR), _c1(1, 2, 9, 4, far)) == "conv1 pair: input (B=1, T=2, idim=9) shorter than the 3x3 kernel"
    bad = _c1(1, 13, 9, 4, far)
    bad.cmvn_mean = _PTR
    assert call(ok, bad) == "conv1 pair: cmvn mean and istd go together"
