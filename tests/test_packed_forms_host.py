"""The packed-row and bf16-row entries (include/m3asr.h "Packed rows"), the part that needs no GPU: the row-plan reference of
tests/packed_ref.py against a brute-force loop, the two host-only name queries, and one refusal per entry that the library
answers on the host, before any launch (csrc/api.hip; operands are placeholders that are never read)."""
import ctypes as C

import numpy as np
import pytest

import packed_ref as R
from m3asr import _lib

T = 9
# the length sets of tests/test_packed_forms_gpu.py (the B = 1024 set is drawn there with the same seed)
LEN_SETS = [[5], [0, 0, 0], [T, T, T], [1, 0, T, 3, 0], [T + 4, -2, 3, T, -1, 0, 2 * T],
            list(np.random.RandomState(7).randint(0, T + 1, size=1024))]
FEAT_SETS = [[6, 7, 11], [4, 6, 7, 11, 3, 43, 39, 0, -5, 200], list(np.random.RandomState(8).randint(0, 48, size=1024))]


@pytest.mark.parametrize("lens", LEN_SETS, ids=lambda l: "B%d" % len(l))
def test_row_plan_reference_is_the_brute_force_plan(lens):
    len_out, row0, pad_of, P = R.row_plan(lens, T)
    b_len, b_row0, b_pad, b_P = R.row_plan_brute(lens, T)
    assert list(len_out) == b_len == [int(l) for l in lens] and list(row0) == b_row0 and list(pad_of) == b_pad and P == b_P
    assert P == sum(min(max(int(l), 0), T) for l in lens) and all(p == -1 for p in pad_of[P:]) and len(pad_of) == len(lens) * T


@pytest.mark.parametrize("feat", FEAT_SETS, ids=lambda l: "B%d" % len(l))
def test_row_plan_reference_with_feature_lengths(feat):
    len_out, row0, pad_of, P = R.row_plan(None, T, feat_len=feat)
    b_len, b_row0, b_pad, b_P = R.row_plan_brute(None, T, feat_len=feat)
    assert list(len_out) == b_len and list(row0) == b_row0 and list(pad_of) == b_pad and P == b_P


def test_subsampled_lengths_are_c_arithmetic():
    """The plan forms ((l - 3) / 2 + 1 - 3) / 2 + 1 with C's truncating division, as oracle.encoder_ref.sub_len documents (the
    plugin's arithmetic): 6, 7 and 11 raw frames give 1, 1 and 2 (floor division would give 0 for 6), and 0 is what l <= 4 gives."""
    from oracle.encoder_ref import sub_len
    import torch
    ls = list(range(-6, 60))
    assert list(R.sub_len(ls)) == [int(v) for v in sub_len(torch.tensor(ls))]
    assert list(R.sub_len([6, 7, 11, 4, 3])) == [1, 1, 2, 0, 0]


def test_pack_and_unpack_reference_round_trip():
    import torch
    lens = [1, 0, T, 3, 0]
    _, row0, pad_of, P = R.row_plan(lens, T)
    padded = torch.arange(len(lens) * T * 2, dtype=torch.float32).view(len(lens) * T, 2) + 1.0
    packed = R.pack(padded, pad_of, P)
    assert packed.shape[0] == P == 13
    back = R.unpack(packed, row0, len(lens), T)
    live = (torch.arange(T).view(1, -1) < torch.tensor(lens).clamp(0, T).view(-1, 1)).reshape(-1)
    assert bool(torch.equal(back[live], padded[live])) and bool((back[~live] == 0).all())


# ---------------------------------------------------------------------------------------- host-only name queries
_HOST = (C.c_char * 4096)()
_PTR = (C.addressof(_HOST) + 15) // 16 * 16


def _linear_desc(M, N, K, w16=False, a16=False):
    d = _lib.LinearDesc()
    d.a, d.lda, d.w, d.y, d.ldy, d.M, d.N, d.K, d.alpha = _PTR, K, _PTR, _PTR, N, M, N, K, 1.0
    d.weight_dtype = _lib.BF16 if w16 else _lib.F32
    d.a_dtype = _lib.BF16 if a16 else _lib.F32
    return d


# the shapes of the GEMM cases in tests/test_packed_forms_gpu.py and the kernel each must reach
LIVE_ROW_SHAPES = [((200, 64, 64, False, False), "gemm_f32_kernel"), ((200, 64, 64, True, False), "gemm_bf16w_kernel"),
                   ((384, 2048, 64, False, False), "gemm_f32_tiled_kernel"), ((1664, 2048, 64, False, False), "gemm_f32_tiled_kernel"),
                   ((384, 2048, 128, True, False), "gemm_bf16w_tiled_kernel"), ((384, 2048, 128, True, True), "gemm_bf16w_tiled_kernel"),
                   ((4096, 128, 64, True, True), "gemm_bf16_dma_kernel")]


@pytest.mark.parametrize("shape,kernel", LIVE_ROW_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(str(int(s)) for s in v))
def test_live_rows_kernel_query_is_the_linear_query(shape, kernel):
    lib = _lib.load()
    d = _linear_desc(*shape)
    for ws in (0, 1):
        assert lib.m3_linear_live_rows_kernel(C.byref(d), ws) == lib.m3_linear_kernel(C.byref(d), ws)
    assert lib.m3_linear_live_rows_kernel(C.byref(d), 0).decode() == kernel


def _conv_kernel(B, T1, F1, Cc, act=1, w16=0, ws=0):
    name = _lib.load().m3_conv2d_3x3s2_kernel(B, T1, F1, Cc, act, w16, ws)
    return name.decode() if name else None


def test_conv2d_kernel_query():
    """The implicit conv's plan: rows = B * T2 * F2, one 64-column tile per 64 channels.  The shapes of the conv_len cases are the
    smallest that the tiled kernels take with four utterances (160 tiles of 64 x 64: plan_gemm); one output frame less per
    utterance and the skinny kernels run them."""
    assert _conv_kernel(4, 81, 131, 64) == "gemm_f32_tiled_kernel"            # 4 * 40 * 65 = 10400 rows = 163 row tiles
    assert _conv_kernel(4, 79, 131, 64) == "gemm_f32_kernel"                  # 4 * 39 * 65 = 10140 rows = 159 row tiles
    assert _conv_kernel(4, 41, 131, 128, w16=1) == "gemm_bf16w_tiled_kernel"  # 5200 rows = 82 row tiles x 2 column tiles
    assert _conv_kernel(4, 39, 131, 128, w16=1) == "gemm_bf16w_kernel"        # 4940 rows = 78 row tiles x 2
    assert _conv_kernel(4, 41, 131, 64, w16=1) == "gemm_bf16w_kernel"         # C % 128 != 0
    assert _conv_kernel(1, 103, 19, 512, ws=1) == "gemm_f32_splitk_kernel" and _conv_kernel(1, 103, 19, 512, ws=0) != "gemm_f32_splitk_kernel"
    assert _conv_kernel(1, 2, 19, 64) is None and "smaller than the kernel" in _lib.last_error()
    assert _conv_kernel(1, 41, 41, 24) is None and "multiple of 16" in _lib.last_error()
    assert _conv_kernel(1, 41, 41, 64, act=3) is None


# ---------------------------------------------------------------------------------------- refusals, one (at least) per entry
def _att_desc(**kw):
    d = _lib.AttentionDesc()
    d.qkv, d.ldq, d.p, d.ldp, d.pos_u, d.pos_v, d.len, d.out, d.ldo = _PTR, 3 * 128, _PTR, 128, _PTR, _PTR, _PTR, _PTR, 128
    d.B, d.T, d.H, d.dk, d.scale = 2, 33, 2, 64, 0.125
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _dw_desc(**kw):
    d = _lib.DwconvDesc()
    d.z, d.w_kc, d.bias, d.gamma, d.beta, d.out, d.eps = _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, 1e-5
    d.B, d.T, d.D, d.K = 2, 20, 512, 15
    for k, v in kw.items():
        setattr(d, k, v)
    return d


class _Lazy:
    """the library, loaded at the first call (collecting this module must not need it)"""

    def __getattr__(self, name):
        return getattr(_lib.load(), name)


def _bad_lda(lib):
    d = _linear_desc(200, 64, 64)
    d.lda = 62
    return lib.m3_linear_live_rows(C.byref(d), _PTR, None, 0, None)


def _refusals():
    lib = _Lazy()
    P, N = _PTR, None
    d = _linear_desc(200, 64, 64)
    return [
        ("pack_plan/null row0", lambda: lib.m3_pack_plan(P, 3, T, N, P, N, N), "null"),
        ("pack_plan/misaligned", lambda: lib.m3_pack_plan(P + 2, 3, T, P, P, N, N), "aligned"),
        ("pack_plan/B over the limit", lambda: lib.m3_pack_plan(P, 1025, T, P, P, N, N), "out of range"),
        ("pack_plan/B = 0", lambda: lib.m3_pack_plan(P, 0, T, P, P, N, N), "out of range"),
        ("unpack_rows/n = 0", lambda: lib.m3_unpack_rows(P, P, 3, T, 0, P, N), "bad sizes"),
        ("unpack_rows/null", lambda: lib.m3_unpack_rows(P, N, 3, T, 4, P, N), "null"),
        ("linear_live_rows/null count", lambda: lib.m3_linear_live_rows(C.byref(d), N, N, 0, N), "live_rows_dev"),
        ("linear_live_rows/misaligned count", lambda: lib.m3_linear_live_rows(C.byref(d), P + 2, N, 0, N), "live_rows_dev"),
        ("linear_live_rows/bad lda", lambda: _bad_lda(lib), "lda"),
        ("router_live_rows/null count", lambda: lib.m3_moe_router_live_rows(P, 64, 64, P, 64, 64, P, N, P, P, 1e-5, P, 64, P, 32, 200, 32, N, N),
         "live_rows_dev"),
        ("router_live_rows/short ldx", lambda: lib.m3_moe_router_live_rows(P, 64, 64, P, 60, 64, P, N, P, P, 1e-5, P, 64, P, 32, 200, 32, P, N), "ldx"),
        ("conv2d_frames/misaligned in", lambda: lib.m3_conv2d_3x3s2_frames(P + 4, P, P, 4, 81, 131, 64, 1, P, 0, P, N), "aligned"),
        ("conv2d_frames/null w", lambda: lib.m3_conv2d_3x3s2_frames(P, N, P, 4, 81, 131, 64, 1, P, 0, P, N), "null"),
        ("conv2d_frames/small input", lambda: lib.m3_conv2d_3x3s2_frames(P, P, P, 4, 2, 131, 64, 1, P, 0, P, N), "smaller than the kernel"),
        ("attention_packed/row0 without len", lambda: lib.m3_relpos_attention_packed(C.byref(_att_desc(len=None)), P, 0, N), "need len"),
        ("attention_packed/short ldq", lambda: lib.m3_relpos_attention_packed(C.byref(_att_desc(ldq=3 * 128 - 4)), P, 0, N), "ldq"),
        ("attention_packed/null descriptor", lambda: lib.m3_relpos_attention_packed(N, P, 0, N), "null descriptor"),
        ("attention_bf16_packed/ldq % 8", lambda: lib.m3_relpos_attention_bf16_packed(C.byref(_att_desc(ldq=3 * 128 + 4)), P, N), "multiples of 8"),
        ("attention_bf16_packed/T > 128", lambda: lib.m3_relpos_attention_bf16_packed(C.byref(_att_desc(T=129)), P, N), "bf16 rows"),
        ("attention_bf16_packed/misaligned row0", lambda: lib.m3_relpos_attention_bf16_packed(C.byref(_att_desc()), P + 2, N), "aligned"),
        ("dwconv_packed/pad_of alone", lambda: lib.m3_dwconv_ln_silu_packed(C.byref(_dw_desc()), P, N, N, 0, N), "go together"),
        ("dwconv_packed/GLU on load with bf16 out", lambda: lib.m3_dwconv_ln_silu_packed(C.byref(_dw_desc(ldz=1024)), P, P, P, 1, N), "GLU on load"),
        ("dwconv_packed/GLU on load, causal", lambda: lib.m3_dwconv_ln_silu_packed(C.byref(_dw_desc(ldz=1024, left_fill=P)), P, P, P, 0, N), "GLU on load"),
        ("dwconv_packed/GLU on load, D = 64", lambda: lib.m3_dwconv_ln_silu_packed(C.byref(_dw_desc(ldz=128, D=64)), P, P, P, 0, N), "GLU on load"),
        ("dwconv_packed/misaligned z", lambda: lib.m3_dwconv_ln_silu_packed(C.byref(_dw_desc(z=P + 4)), P, P, P, 0, N), "aligned"),
        ("layer_norm_ex/stats without the bf16 copy", lambda: lib.m3_layer_norm_ex(P, P, P, 1e-5, P, 5, 256, N, P, N, N, 0.0, N, N), "y_stats"),
        ("layer_norm_ex/gamma2 without y2", lambda: lib.m3_layer_norm_ex(P, P, P, 1e-5, P, 5, 256, N, N, P, P, 1e-5, N, N), "second LayerNorm"),
        ("layer_norm_ex/misaligned y_bf16", lambda: lib.m3_layer_norm_ex(P, P, P, 1e-5, P, 5, 256, P + 8, N, N, N, 0.0, N, N), "aligned"),
        ("layer_norm_ex/dim % 4", lambda: lib.m3_layer_norm_ex(P, P, P, 1e-5, P, 5, 258, N, N, N, N, 0.0, N, N), "multiple of 4"),
        ("row_stats_bf16/dim % 8", lambda: lib.m3_row_stats_bf16(P, 5, 516, P, N), "multiple of 8"),
        ("row_stats_bf16/null stats", lambda: lib.m3_row_stats_bf16(P, 5, 512, N, N), "null"),
        ("rows_to_bf16/short ldx", lambda: lib.m3_rows_to_bf16(P, 508, 5, 512, P, N), "ldx"),
        ("rows_to_bf16/misaligned xb", lambda: lib.m3_rows_to_bf16(P, 512, 5, 512, P + 4, N), "aligned"),
    ]


_REFUSALS = _refusals()


@pytest.mark.parametrize("what", [r[0] for r in _REFUSALS])
def test_entry_refuses_on_the_host(what):
    call, word = next((c, w) for n, c, w in _REFUSALS if n == what)
    assert call() != 0, what
    assert word in _lib.last_error(), (what, _lib.last_error())


def test_every_new_entry_has_a_refusal():
    entries = {"pack_plan", "unpack_rows", "linear_live_rows", "router_live_rows", "conv2d_frames", "attention_packed",
               "attention_bf16_packed", "dwconv_packed", "layer_norm_ex", "row_stats_bf16", "rows_to_bf16"}
    assert {n.split("/")[0] for n, _, _ in _REFUSALS} == entries


# ---------------------------------------------------------------------------------------- the other references, against torch
def _rnd(*shape, seed=0):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("causal", [False, True], ids=["symmetric", "causal"])
def test_packed_dwconv_reference_is_the_padded_conv(causal):
    """packed_dwconv_ref against torch's conv1d + layer_norm on the padded batch whose frames >= len hold the pad row"""
    import torch
    import torch.nn.functional as F
    lens, Tt, D, K = [1, 0, 7, 8, 20], 20, 8, 7
    B = len(lens)
    _, row0, pad_of, P = R.row_plan(lens, Tt)
    z, pad_row = _rnd(B * Tt, D, seed=1).double(), _rnd(D, seed=2).double()
    w_kc, bias, gamma, beta, fill = _rnd(K, D, seed=3).double(), _rnd(D, seed=4).double(), _rnd(D, seed=5).double(), _rnd(D, seed=6).double(), _rnd(D, seed=7).double()
    live = (torch.arange(Tt).view(1, -1) < torch.tensor(lens).view(-1, 1)).reshape(-1, 1)
    zp = torch.where(live, z, pad_row.view(1, -1).expand_as(z)).view(B, Tt, D).transpose(1, 2)          # (B, D, T)
    if causal:
        zp = torch.cat([fill.view(1, D, 1).expand(B, D, K - 1), zp], -1)
        y = F.conv1d(zp, w_kc.t().unsqueeze(1), bias, groups=D)
    else:
        y = F.conv1d(zp, w_kc.t().unsqueeze(1), bias, padding=(K - 1) // 2, groups=D)
    y = F.layer_norm(y.transpose(1, 2), (D,), gamma, beta, 1e-5)
    want = R.pack((y * torch.sigmoid(y)).reshape(B * Tt, D), pad_of, P)
    got = R.packed_dwconv_ref(R.pack(z, pad_of, P), pad_row, w_kc, bias, gamma, beta, 1e-5, lens, row0, Tt, left_fill=fill if causal else None)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("chunk,left", [(0, -1), (16, 2), (5, 0)])
def test_packed_attention_reference_is_the_padded_reference(chunk, left):
    """per utterance on its own frames == the padded batch's reference on the valid query rows"""
    import torch
    from stream_kernels_ref import attention_ref
    lens, Tt, H, dk = [16, 1, 0, 17, 15, 33], 33, 2, 16
    B, D = len(lens), H * dk
    _, row0, pad_of, P = R.row_plan(lens, Tt)
    qkv, p, u, v = _rnd(B * Tt, 3 * D, seed=1), _rnd(Tt, D, seed=2), _rnd(H, dk, seed=3) * 0.3, _rnd(H, dk, seed=4) * 0.3
    want = R.pack(attention_ref(qkv, p, u, v, torch.tensor(lens), B, Tt, H, dk, chunk, left), pad_of, P)
    got = R.packed_attention_ref(R.pack(qkv, pad_of, P), p, u, v, lens, row0, Tt, H, dk, chunk, left)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12
