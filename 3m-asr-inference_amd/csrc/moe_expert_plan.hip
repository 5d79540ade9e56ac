// The grouped expert FFN's form, decided once (host only): plan_expert_ffn picks the kernel and lays out the slab region,
// launch_expert_ffn runs the plan.  kernels.h has the table of form against condition.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace m3 {

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

ExpertFfnPlan plan_expert_ffn(ExpertWeights w, int S, int E, int D, int F, unsigned flags) {
  // read once: the engine freezes the form (and the combine's slab layout) when a shape is bound
  static const int tiled_min_rows = env_int("M3_EXPERT_TILED_MIN_ROWS", 1024);
  static const int fused_min_rows = env_int("M3_EXPERT_FUSED_FP8_MIN_ROWS", 4096);
  static const int g256_min_rows_per_expert = env_int("M3_G256_MIN_ROWS_PER_EXPERT", 512);
  const bool f32 = w == ExpertWeights::F32, bf16 = w == ExpertWeights::BF16, w4 = w == ExpertWeights::MXFP4;
  ExpertFfnPlan p{};
  p.weights = w;
  p.label = "";
  if (S <= 0 || E <= 0 || D <= 0 || F <= 0) return p;   // launches = 0: nothing the operator takes
  const size_t room = expert_ffn_slab_bytes(S, D, F);

  if (w == ExpertWeights::FP8A8 && S >= fused_min_rows) {
    if (const int fs = expert_ffn_fused_fp8_fsplit(S, E, D, F)) {
      // its fs slabs of [S][D] fit: F % (128 fs) == 0, so fs <= F / 128 < F / 64, the slab count the region is sized for
      p.kernel = ExpertKernel::FusedFp8; p.label = "expert_ffn_fused_fp8_kernel";
      p.launches = 1; p.slices = p.fsplit = fs;
      return p;
    }
  }
  // two grouped GEMMs: H (fp32 / bf16, S*F) and the sorted result rows (fp32, S*D) in the region the slabs would use
  const size_t h_bytes = align_up((size_t)S * F * (f32 ? 4 : 2), 256), y_bytes = (size_t)S * D * 4;
  const int tile = f32 ? 64 : 128;
  const bool norm_in_kernel = f32 && (flags & EXPERT_NORM_IN_KERNEL);
  if (!norm_in_kernel && S >= tiled_min_rows && D % tile == 0 && F % tile == 0 && h_bytes + y_bytes <= room) {
    p.launches = 2; p.slices = 1; p.rows_off = h_bytes;
    const size_t xb_off = h_bytes + align_up(y_bytes, 256);   // g256 reads bf16 rows: converted once, behind the result rows
    if (bf16 && !(flags & EXPERT_SCATTER_ROWS) && expert_gemm_g256_takes(S, E, D, F) && S / E >= g256_min_rows_per_expert &&
        xb_off + (size_t)S * D * 2 <= room) {
      p.kernel = ExpertKernel::G256Bf16; p.label = "expert_gemm_g256_kernel";
      p.launches = 3; p.xb_off = xb_off;                      // rows -> bf16, GEMM-1, GEMM-2
    } else if (f32) {
      p.kernel = ExpertKernel::TiledF32; p.label = "expert_gemm_f32_tiled_kernel";
    } else {
      p.kernel = bf16 ? ExpertKernel::TiledBf16 : w4 ? ExpertKernel::TiledW4 : ExpertKernel::TiledW8;
      p.label = bf16 ? "gemm_bf16w_tiled_kernel<grouped>" : w4 ? "gemm_bf16w_tiled_kernel<grouped,mxfp4>" : "gemm_bf16w_tiled_kernel<grouped,fp8>";
    }
    return p;
  }
  // one launch, every 64-wide slice of F leaves a partial result: F / 64 slabs of [S][D]
  p.kernel = f32 ? ExpertKernel::SlabF32 : bf16 ? ExpertKernel::SlabBf16 : w4 ? ExpertKernel::SlabW4 : ExpertKernel::SlabW8;
  p.label = f32 ? "expert_ffn_f32_kernel" : bf16 ? "expert_ffn_bf16w_kernel" : w4 ? "expert_ffn_w4_kernel" : "expert_ffn_w8_kernel";
  const int slice = f32 ? kExpertSlice : kExpertSliceW16, d_mult = f32 ? 16 : bf16 ? 32 : w4 ? 128 : 64;
  p.slices = F / slice;
  p.launches = D % d_mult == 0 && D <= 2048 && F % slice == 0 ? 1 : 0;   // 0: dimensions the slab launchers reject (they say why)
  return p;
}

int launch_expert_ffn(const ExpertFfnPlan& plan, int S, int E, int D, int F, const ExpertFfnArgs& a, hipStream_t stream) {
  M3_REQUIRE(a.ln_gamma == nullptr || plan.kernel == ExpertKernel::SlabF32, "expert_ffn: LayerNorm while gathering exists in the fp32 slab form only (S=%d E=%d)", S, E);
  M3_REQUIRE(a.y_scatter == nullptr || plan.kernel == ExpertKernel::TiledBf16, "expert_ffn: the scattering epilogue exists in the bf16 tiled form only (S=%d E=%d)", S, E);
  M3_REQUIRE(a.w2_sliced != EXPERT_W_FRAG || plan.kernel == ExpertKernel::SlabF32,
             "expert_ffn: fragment-ordered weights exist for the fp32 slab form only; S=%d E=%d D=%d F=%d runs %s", S, E, D, F, plan.label);
  char* const region = (char*)a.slab;
  void* const hbuf = region + plan.h_off;
  float* const ybuf = (float*)(region + plan.rows_off);
  switch (plan.kernel) {
    case ExpertKernel::SlabF32:
      return launch_expert_ffn_f32_slab(a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, (const float*)a.w1, a.b1, (const float*)a.w2, a.w2_sliced,
                                        ybuf, a.ln_gamma, a.ln_beta, a.ln_eps, stream);
    case ExpertKernel::TiledF32:
      return launch_expert_tiled_f32(a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, (const float*)a.w1, a.b1, (const float*)a.w2, a.w2_sliced,
                                     (float*)hbuf, ybuf, stream);
    case ExpertKernel::SlabBf16:
      return launch_expert_ffn_bf16w_slab(a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, a.b1, a.w2, a.w2_sliced, ybuf, stream);
    case ExpertKernel::TiledBf16:
      return launch_expert_tiled_w16(0, a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, nullptr, a.b1, a.w2, nullptr, a.w2_sliced,
                                     hbuf, ybuf, stream, a.b2, a.y_scatter);
    case ExpertKernel::G256Bf16: {
      void* const xb = region + plan.xb_off;
      if (int rc = launch_rows_to_bf16(a.x, a.ldx, S, D, xb, stream)) return rc;
      return launch_expert_ffn_bf16_g256(xb, D, a.pos, a.acc_hist, S, E, D, F, a.w1, a.b1, a.w2, a.w2_sliced, hbuf, ybuf, stream);
    }
    case ExpertKernel::SlabW8:
      return launch_expert_ffn_w8_slab(a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, a.s1, a.b1, a.w2, a.s2, a.w2_sliced, ybuf, stream);
    case ExpertKernel::TiledW8:
      return launch_expert_tiled_w16(1, a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, a.s1, a.b1, a.w2, a.s2, a.w2_sliced, hbuf,
                                     ybuf, stream);
    case ExpertKernel::SlabW4:
      return launch_expert_ffn_w4_slab(a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, a.s1, a.b1, a.w2, a.s2, a.w2_sliced, ybuf, stream);
    case ExpertKernel::TiledW4:
      return launch_expert_tiled_w16(2, a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, a.s1, a.b1, a.w2, a.s2, a.w2_sliced, hbuf,
                                     ybuf, stream);
    case ExpertKernel::FusedFp8:
      // (xq / xq_scale: only this kernel takes them; x stays valid for the other forms)
      return launch_expert_ffn_fused_fp8(a.x, a.ldx, a.pos, a.acc_hist, S, E, D, F, a.w1, a.s1, a.b1, a.w2, a.s2, a.w2_sliced, a.h_scale,
                                         plan.fsplit, ybuf, stream, a.xq, a.xq_scale, a.fs_dev);
  }
  return -2;
}

}  // namespace m3
