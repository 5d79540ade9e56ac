"""The grouped expert FFN's form is decided in one place (plan_expert_ffn, csrc/moe_expert_plan.hip).  This table pins what it
answers, through the host-only entry m3_moe_expert_ffn_kernel; no GPU is needed (without a device the library assumes 256
CUs, the MI355X's count, for the fused fp8 kernel's F-split cost model).

How the expected column was obtained: NOT from the planner.  The commit before the planner existed exported its free
predicates with C++ linkage (m3::expert_ffn_f32_tiled / _slices, m3::expert_ffn_w16_kernel / _launches / _slices(wmode, ...));
a scratch script built that commit's library, called them through ctypes by their mangled names for every row below and
printed the rows.  fp32 rows: label and launch count as engine.hip's expert_form derived them from expert_ffn_f32_tiled.

The boundaries, each from both sides: 1023 / 1024 rows (M3_EXPERT_TILED_MIN_ROWS); the tile multiples of D (64 for fp32, 128
for bf16 / fp8: D = 192 tiles in fp32 only; at D = 64 fp32 stays with the slabs as well, because H = S*F*4 bytes alone is
the whole slab region F/64 * S*64*4, while D = 128 tiles in both); F = 1088 (a multiple of 64 but not of 128: slab at 5000
rows in the 16-bit forms); 511 / 512 rows per expert with D, F multiples of 256, D or F not a multiple of 256, and E = 128
(g256); 4095 / 4096 rows with S >= 64 E on both sides, 8191 / 8192 rows at E = 128 and S < 64 E (fused fp8); F = 128, 1024,
2048, 4096 (the F split in the slices column), 4224 (> 4096) and 192 (not a multiple of 128) falling back; D = 256 under
fp8 arithmetic (weight-only); one utterance (S = 50, E = 32) in every dtype."""
import ctypes as C

import pytest

from m3asr import _lib

DT = {"f32": 0, "bf16": 4, "fp8": 5}    # m3_dtype (include/m3asr.h)

# ((weight dtype, fp8_activations, S, E, D, F), (kernel label, launches, partial-result slabs))
TABLE = [
    (("f32", 0, 50, 32, 512, 1024), ("expert_ffn_f32_kernel", 1, 16)),
    (("bf16", 0, 50, 32, 512, 1024), ("expert_ffn_bf16w_kernel", 1, 16)),
    (("fp8", 0, 50, 32, 512, 1024), ("expert_ffn_w8_kernel", 1, 16)),
    (("fp8", 1, 50, 32, 512, 1024), ("expert_ffn_w8_kernel", 1, 16)),
    (("f32", 0, 1023, 32, 512, 1024), ("expert_ffn_f32_kernel", 1, 16)),
    (("f32", 0, 1024, 32, 512, 1024), ("expert_gemm_f32_tiled_kernel", 2, 1)),
    (("bf16", 0, 1023, 32, 512, 1024), ("expert_ffn_bf16w_kernel", 1, 16)),
    (("bf16", 0, 1024, 32, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped>", 2, 1)),
    (("fp8", 0, 1023, 32, 512, 1024), ("expert_ffn_w8_kernel", 1, 16)),
    (("fp8", 0, 1024, 32, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 1, 1023, 32, 512, 1024), ("expert_ffn_w8_kernel", 1, 16)),
    (("fp8", 1, 1024, 32, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("f32", 0, 2048, 8, 64, 256), ("expert_ffn_f32_kernel", 1, 4)),
    (("bf16", 0, 2048, 8, 64, 256), ("expert_ffn_bf16w_kernel", 1, 4)),
    (("fp8", 0, 2048, 8, 64, 256), ("expert_ffn_w8_kernel", 1, 4)),
    (("f32", 0, 2048, 8, 192, 256), ("expert_gemm_f32_tiled_kernel", 2, 1)),
    (("bf16", 0, 2048, 8, 128, 256), ("gemm_bf16w_tiled_kernel<grouped>", 2, 1)),
    (("bf16", 0, 2048, 8, 192, 256), ("expert_ffn_bf16w_kernel", 1, 4)),
    (("fp8", 0, 2048, 8, 192, 256), ("expert_ffn_w8_kernel", 1, 4)),
    (("f32", 0, 2048, 8, 128, 256), ("expert_gemm_f32_tiled_kernel", 2, 1)),
    (("f32", 0, 5000, 32, 512, 1088), ("expert_gemm_f32_tiled_kernel", 2, 1)),
    (("bf16", 0, 5000, 32, 512, 1088), ("expert_ffn_bf16w_kernel", 1, 17)),
    (("fp8", 0, 5000, 32, 512, 1088), ("expert_ffn_w8_kernel", 1, 17)),
    (("fp8", 1, 5000, 32, 512, 1088), ("expert_ffn_w8_kernel", 1, 17)),
    (("bf16", 0, 4088, 8, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped>", 2, 1)),
    (("bf16", 0, 4096, 8, 512, 1024), ("expert_gemm_g256_kernel", 3, 1)),
    (("bf16", 0, 4096, 8, 384, 1024), ("gemm_bf16w_tiled_kernel<grouped>", 2, 1)),
    (("bf16", 0, 4096, 8, 512, 1152), ("gemm_bf16w_tiled_kernel<grouped>", 2, 1)),
    (("bf16", 0, 65536, 128, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped>", 2, 1)),
    (("bf16", 0, 32768, 64, 512, 1024), ("expert_gemm_g256_kernel", 3, 1)),
    (("fp8", 1, 4095, 32, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 1, 4096, 32, 512, 1024), ("expert_ffn_fused_fp8_kernel", 1, 4)),
    (("fp8", 1, 4095, 64, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 1, 4096, 64, 512, 1024), ("expert_ffn_fused_fp8_kernel", 1, 4)),
    (("fp8", 1, 8191, 128, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 1, 8192, 128, 512, 1024), ("expert_ffn_fused_fp8_kernel", 1, 2)),
    (("fp8", 1, 4096, 128, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 1, 8192, 32, 512, 128), ("expert_ffn_fused_fp8_kernel", 1, 1)),
    (("fp8", 1, 8192, 32, 512, 1024), ("expert_ffn_fused_fp8_kernel", 1, 2)),
    (("fp8", 1, 8192, 32, 512, 2048), ("expert_ffn_fused_fp8_kernel", 1, 2)),
    (("fp8", 1, 8192, 32, 512, 4096), ("expert_ffn_fused_fp8_kernel", 1, 4)),
    (("fp8", 1, 8192, 32, 512, 4224), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 1, 8192, 32, 512, 192), ("expert_ffn_w8_kernel", 1, 3)),
    (("fp8", 1, 8192, 32, 256, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("fp8", 0, 8192, 32, 512, 1024), ("gemm_bf16w_tiled_kernel<grouped,fp8>", 2, 1)),
    (("f32", 0, 8192, 32, 512, 1024), ("expert_gemm_f32_tiled_kernel", 2, 1)),
    (("fp8", 1, 40000, 64, 512, 1024), ("expert_ffn_fused_fp8_kernel", 1, 1)),
]
ALL_LABELS = {"expert_ffn_f32_kernel", "expert_gemm_f32_tiled_kernel", "expert_ffn_bf16w_kernel", "gemm_bf16w_tiled_kernel<grouped>",
              "expert_gemm_g256_kernel", "expert_ffn_w8_kernel", "gemm_bf16w_tiled_kernel<grouped,fp8>", "expert_ffn_fused_fp8_kernel"}


def _query(lib, dt, a8, S, E, D, F):
    launches, slices = C.c_int32(-1), C.c_int32(-1)
    label = lib.m3_moe_expert_ffn_kernel(DT[dt], a8, S, E, D, F, C.byref(launches), C.byref(slices))
    return (label.decode() if label is not None else None, launches.value, slices.value)


def test_table_covers_every_form():
    """what keeps the table from silently covering less: all eight ExpertKernel labels are expected somewhere"""
    assert {want[0] for _, want in TABLE} == ALL_LABELS
    assert len(set(case for case, _ in TABLE)) == len(TABLE)


@pytest.mark.parametrize("case,want", TABLE, ids=["%s%s-S%d-E%d-D%d-F%d" % (c[0], "a8" if c[1] else "", *c[2:]) for c, _ in TABLE])
def test_form_matches_the_predicates_it_replaced(case, want):
    lib = _lib.load()
    assert _query(lib, *case) == want
    dt, a8, S, E, D, F = case
    if dt == "fp8" and a8:   # one question, one spelling: "active" is "the plan runs the fused kernel"
        assert lib.m3_moe_expert_ffn_fp8a8_active(S, E, D, F) == int(want[0] == "expert_ffn_fused_fp8_kernel")


def test_rejected_shapes_and_null_outputs():
    lib = _lib.load()
    assert _query(lib, "f32", 0, 50, 32, 528, 1024) == ("expert_ffn_f32_kernel", 1, 16)     # idim % 16 == 0 is all fp32 asks
    for bad in [("f32", 0, 50, 32, 500, 1024), ("bf16", 0, 50, 32, 528, 1024), ("fp8", 0, 50, 32, 544, 1024), ("fp8", 1, 50, 32, 544, 1024),
                ("f32", 0, 50, 32, 512, 1000), ("bf16", 0, 50, 32, 512, 1056), ("f32", 0, 0, 32, 512, 1024), ("f32", 0, 50, 0, 512, 1024),
                ("f32", 0, 50, 32, 4096, 1024), ("f32", 1, 50, 32, 512, 1024), ("bf16", 1, 50, 32, 512, 1024)]:
        assert _query(lib, *bad) == (None, -1, -1), bad
    assert lib.m3_moe_expert_ffn_kernel(1, 0, 50, 32, 512, 1024, None, None) is None        # M3_F16: not an expert weight dtype
    assert lib.m3_moe_expert_ffn_kernel(4, 0, 4096, 8, 512, 1024, None, None) == b"expert_gemm_g256_kernel"


class _Plan(C.Structure):    # m3::ExpertFfnPlan (csrc/kernels.h)
    _fields_ = [("weights", C.c_int), ("kernel", C.c_int), ("label", C.c_char_p), ("launches", C.c_int), ("slices", C.c_int),
                ("fsplit", C.c_int), ("h_off", C.c_size_t), ("rows_off", C.c_size_t), ("xb_off", C.c_size_t)]


F32, BF16, FP8, FP8A8 = range(4)                          # m3::ExpertWeights
NORM_IN_KERNEL, SCATTER_ROWS = 1, 2                       # EXPERT_NORM_IN_KERNEL, EXPERT_SCATTER_ROWS
SLAB_F32, TILED_F32, SLAB_BF16, TILED_BF16, G256_BF16, SLAB_W8, TILED_W8, FUSED_FP8 = range(8)   # m3::ExpertKernel


def _plan(w, S, E, D, F, flags=0):
    """m3::plan_expert_ffn itself (C++ linkage: the C entry has no flags argument)"""
    fn = C.CDLL(_lib.LIB_PATH)["_ZN2m315plan_expert_ffnENS_13ExpertWeightsEiiiij"]
    fn.restype = _Plan
    fn.argtypes = [C.c_int] * 5 + [C.c_uint]
    return fn(w, S, E, D, F, flags)


def _align(v):
    return (v + 255) // 256 * 256


def test_flags_and_slab_layout():
    S, E, D, F = 4096, 8, 512, 1024                       # g256-eligible: 512 rows per expert, D and F multiples of 256
    room = F // 64 * S * D * 4                            # expert_ffn_slab_bytes
    p = _plan(BF16, S, E, D, F)
    assert (p.kernel, p.label, p.launches, p.slices) == (G256_BF16, b"expert_gemm_g256_kernel", 3, 1)
    assert (p.h_off, p.rows_off, p.xb_off) == (0, _align(S * F * 2), _align(S * F * 2) + _align(S * D * 4))
    assert p.xb_off + S * D * 2 <= room                   # the bf16 row copy is inside the region too
    # the expert-parallel receive side scatters from GEMM-2's epilogue, which the g256 kernel does not have: tiled, 2 launches
    p = _plan(BF16, S, E, D, F, SCATTER_ROWS)
    assert (p.kernel, p.label, p.launches, p.slices) == (TILED_BF16, b"gemm_bf16w_tiled_kernel<grouped>", 2, 1)
    assert (p.h_off, p.rows_off, p.xb_off) == (0, _align(S * F * 2), 0)
    # ... and changes nothing for the other dtypes or below the tiled form
    assert _plan(F32, S, E, D, F, SCATTER_ROWS).kernel == TILED_F32 and _plan(FP8, S, E, D, F, SCATTER_ROWS).kernel == TILED_W8
    assert _plan(FP8A8, S, E, D, F, SCATTER_ROWS).kernel == FUSED_FP8
    assert _plan(BF16, 1023, E, D, F, SCATTER_ROWS).kernel == SLAB_BF16
    # norm_ff applied while the rows are gathered exists in the fp32 slab kernel only
    p = _plan(F32, 2048, 32, D, F)
    assert (p.kernel, p.launches, p.slices, p.rows_off) == (TILED_F32, 2, 1, _align(2048 * F * 4))
    p = _plan(F32, 2048, 32, D, F, NORM_IN_KERNEL)
    assert (p.kernel, p.label, p.launches, p.slices) == (SLAB_F32, b"expert_ffn_f32_kernel", 1, F // 64)
    assert (p.h_off, p.rows_off, p.xb_off) == (0, 0, 0)
    # the fused fp8 kernel: fsplit slabs at the start of the region
    p = _plan(FP8A8, 8192, 32, 512, 2048)
    assert (p.kernel, p.launches, p.slices, p.fsplit, p.rows_off) == (FUSED_FP8, 1, 2, 2, 0)
    assert p.slices * 8192 * 512 * 4 <= 2048 // 64 * 8192 * 512 * 4
