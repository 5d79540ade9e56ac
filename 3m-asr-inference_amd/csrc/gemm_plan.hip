// The dense GEMM's form, decided once (host only): plan_gemm checks the operands and picks the kernel, its instantiation, its
// grid and its workspace; launch_gemm runs the record of the two (GemmLaunch).  kernels.h has the table of form against condition.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace m3 {

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// a condition a problem must meet: otherwise the plan keeps launches = 0 and says why
#define M3_PLAN_REQUIRE(cond, ...)                                  \
  do {                                                              \
    if (!(cond)) {                                                  \
      snprintf(plan.reason, sizeof(plan.reason), __VA_ARGS__);      \
      return false;                                                 \
    }                                                               \
  } while (0)

// what every kernel of the family asks of its operands (`who`: the name the messages carry, by weight dtype)
static bool operands_ok(const GemmParams& p, const char* who, GemmPlan& plan) {
  const int kmult = p.w_bf16 ? 32 : 16;   // one MFMA step of the skinny kernels
  M3_PLAN_REQUIRE(p.grp_acc == nullptr, "%s: grouped (per-expert) operands belong to the expert FFN's plan", who);
  M3_PLAN_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "%s: empty problem M=%d N=%d K=%d", who, p.M, p.N, p.K);
  M3_PLAN_REQUIRE(p.K % kmult == 0, "%s: K=%d must be a multiple of %d", who, p.K, kmult);
  M3_PLAN_REQUIRE((p.lda & 3) == 0, "%s: lda=%d must be a multiple of 4", who, p.lda);
  M3_PLAN_REQUIRE(!plan.glu || (p.N & 1) == 0, "%s: GLU needs even N", who);
  if (plan.conv) {
    M3_PLAN_REQUIRE(p.conv_C % kmult == 0 && p.K == 9 * p.conv_C, "%s: conv mode needs K=9*C, C%%%d==0", who, kmult);
    M3_PLAN_REQUIRE(!plan.glu && plan.ln == GEMM_LN_NONE, "%s: conv mode supports neither GLU nor LayerNorm", who);
  }
  M3_PLAN_REQUIRE(!(p.ln_wsum && p.mask_in) || p.ln_wbeta, "%s: folded LayerNorm + input mask needs ln_wbeta", who);
  if (p.mask_in || p.mask_out) M3_PLAN_REQUIRE(p.row_len && p.rows_per_batch > 0, "%s: mask needs row_len", who);
  return true;
}

// deep, narrow fp32 problems (few output tiles, long K, plain epilogue): K ranges and the workspace their partial tiles need
static int splitk_ranges(const GemmParams& p, size_t* ws_bytes) {
  if (p.w_bf16 || p.K < 4096 || (p.K & 63) || (p.N & 3) || (p.lda & 3) || (p.ldy & 3)) return 0;
  if (p.mode == GEMM_A_CONCAT2 || p.ln_wsum || p.ln_gamma || p.mask_in || p.mask_out || p.resid || p.act == ACT_GLU) return 0;
  if (p.mode == GEMM_A_CONV3X3S2 && (p.conv_C & 63)) return 0;
  const long tiles = (long)cdiv(p.M, 64) * cdiv(p.N, 64);
  if (tiles > 160) return 0;                          // enough tiles: the other kernels fill the chip
  const int nsteps = p.K / 64;
  int splits = (int)(512 / tiles);                    // ~2 workgroups per CU
  if (splits > nsteps / 4) splits = nsteps / 4;       // >= 4 k-steps per workgroup
  if (splits < 2) return 0;
  splits = cdiv(nsteps, cdiv(nsteps, splits));
  *ws_bytes = (size_t)splits * p.M * p.N * sizeof(float);
  return splits;
}

// the LDS-tiled kernels' grid: row tiles in groups of 8 (one per XCD), GLU tiles hold bn / 2 value + bn / 2 gate columns
static void tiled_grid(const GemmParams& p, GemmPlan& plan, int bm, int bn, int bk) {
  plan.bm = bm; plan.bn = bn; plan.bk = bk;
  plan.m_tiles = cdiv(p.M, bm);
  plan.n_tiles = plan.glu ? cdiv(p.N / 2, bn / 2) : cdiv(p.N, bn);
}

// the skinny kernels' row tile: 16 * mt rows per workgroup; short inputs are cut into 16-row tiles to fill the chip, but more
// workgroups than fit at once (2 per CU) only serialise: then prefer fatter tiles
static void skinny_grid(const GemmParams& p, GemmPlan& plan, int Nout) {
  int mt = p.M <= 128 ? 1 : (p.M <= 512 ? 2 : 4);
  while (mt < 4 && 16 * mt < p.M && (long)cdiv(Nout, 16) * cdiv(p.M, 16 * mt) > 512) mt *= 2;
  // narrow outputs over many rows (the router: N = 32 experts, S ~ 2000 rows): fat row tiles would leave most CUs idle
  while (!p.w_bf16 && mt > 1 && (long)cdiv(Nout, 16) * cdiv(p.M, 16 * mt) < 256) mt /= 2;
  plan.mt = mt;
  plan.n_tiles = cdiv(Nout, 16);
  plan.m_tiles = cdiv(p.M, 16 * mt);
  plan.xcd_swizzle = (plan.n_tiles % 8 == 0) ? 1 : 0;
  plan.nw = p.K >= 2048 ? 16 : (p.K >= 1024 ? 8 : 4);
  if (plan.nw == 16 && (plan.glu || mt == 4 || plan.ln != GEMM_LN_NONE)) plan.nw = 8;   // those 16-wave variants would spill registers
  const int steps = p.w_bf16 ? (p.K >> 5) : (p.K >> 4);
  const int group = p.w_bf16 ? gemm16_group_steps(mt, plan.nw) : gemm_group_steps(mt, plan.glu ? 2 : 1, plan.nw);
  plan.nbuf = steps <= plan.nw * group ? 1 : 2;
}

static bool choose_form(const GemmParams& p, size_t ws_avail, GemmPlan& plan) {
  // read once: the engine freezes the form when a shape is bound.  Below tiled_min_rows rows the K-split kernels fill the chip
  // better.  dma_min_rows: measured against the register-staged kernel (tools/bench_gemm_bf16.py --a16,
  // profiles/r03_gemm_dma_vs_staged.txt): +12-16 % at 16 384 rows, +0-16 % at 4 480, SLOWER at 1 984 rows (128 x 128 tiles leave
  // most CUs idle there and a CU keeps only ~16 KB of LDS-DMA in flight: a k-step is a full ~1.3 us round trip).
  static const int tiled_min_rows = env_int("M3_TILED_MIN_ROWS", 384);
  static const int dma_min_rows = env_int("M3_DMA_MIN_ROWS", 4096);
  static const int thin_below = env_int("M3_TILED_THIN_BELOW", 0);
  const bool glu = plan.glu, conv = plan.conv, concat = p.mode == GEMM_A_CONCAT2;
  const int Nout = glu ? p.N / 2 : p.N;
  const long tiles64 = (long)cdiv(p.M, 64) * cdiv(Nout, 64);
  // the LDS-tiled kernels need enough 64 x 64 tiles to occupy the chip: below ~160 the K-split kernels' many small workgroups win
  const bool long_batch = p.M >= tiled_min_rows && tiles64 >= 160 && !concat && p.ln_gamma == nullptr;
  const bool big = (long)cdiv(p.M, 128) * cdiv(p.N, 128) >= 200;   // 128 x 128 tiles when >= ~200 of them exist (MFMA-heavy: conv2)

  size_t need = 0;
  if (const int splits = splitk_ranges(p, &need); splits >= 2 && ws_avail >= need) {
    plan.kernel = GemmKernel::SplitKF32; plan.label = "gemm_f32_splitk_kernel";
    plan.splits = splits; plan.ws_bytes = need;
    plan.bm = plan.bn = plan.bk = 64;
    plan.m_tiles = cdiv(p.M, 64); plan.n_tiles = cdiv(p.N, 64);
    return true;
  }
  if (p.w_bf16) {
    const char* who = "gemm_bf16w";
    M3_PLAN_REQUIRE(!concat, "%s: concat operands are fp32-only (the router stays fp32)", who);
    M3_PLAN_REQUIRE(p.ln_gamma == nullptr && p.ln_out == nullptr, "%s: only the folded LayerNorm (ln_wsum) is available with bf16 weights", who);
    if (plan.ln) M3_PLAN_REQUIRE(p.mode == GEMM_A_PLAIN && p.K <= 2047, "%s: LayerNorm needs plain A with K < 2048", who);
    const bool bf16_out_ok = (Nout & 3) == 0 && (p.ldy & 3) == 0 && (p.ldyb & 3) == 0;
    // plain row-major bf16 A, K a multiple of the k-step, 32-bit buffer offsets, folded LayerNorm only with the producer's row statistics
    if (p.M >= dma_min_rows && p.a_bf16 && p.mode == GEMM_A_PLAIN && p.w_scale == nullptr && (p.K & 63) == 0 && (p.lda & 7) == 0 &&
        (p.ln_wsum == nullptr || p.ln_stats != nullptr) && ((size_t)(p.M - 1) * p.lda + p.K) * 2 < ((size_t)1 << 32) &&
        (size_t)p.N * p.K * 2 < ((size_t)1 << 32)) {
      M3_PLAN_REQUIRE(!(p.y_bf16 || p.Yb) || bf16_out_ok, "gemm_bf16_dma: bf16 output needs N %% 4 == 0");
      plan.kernel = GemmKernel::DmaBf16; plan.label = "gemm_bf16_dma_kernel";
      tiled_grid(p, plan, 128, 128, 64);
      // work-groups that do not outnumber the CUs: one per CU with a 4-stage ring; else two per CU with 2 stages each
      plan.stages = (long)plan.m_tiles * plan.n_tiles <= device_cu_count() && p.K / 64 >= 4 ? 4 : 2;
      return true;
    }
    // only the LDS-DMA kernel writes / reads the row-statistic partials: a consumer of y_copy_stats would read stale numbers
    M3_PLAN_REQUIRE(p.Yb_stats == nullptr && p.ln_stats == nullptr,
                    "%s: y_copy_stats / ln_stats need the LDS-DMA kernel (M >= %d rows, bf16 A); this problem (M=%d) runs on another one",
                    who, dma_min_rows, p.M);
    if (long_batch && (p.K & 127) == 0 && (!conv || (p.conv_C & 127) == 0)) {
      if (p.a_bf16 && !conv) M3_PLAN_REQUIRE((p.lda & 7) == 0, "%s: bf16 A needs lda %% 8 == 0", who);
      M3_PLAN_REQUIRE(!(p.y_bf16 || p.Yb) || bf16_out_ok, "%s: bf16 output needs N %% 4 == 0", who);
      plan.kernel = GemmKernel::TiledBf16; plan.label = "gemm_bf16w_tiled_kernel";
      // else 64 x 64 x 128: 4x the workgroups and half the k-steps, because a small GEMM is a chain of k-steps of ~1 us memory
      // latency each.  Few 64 x 64 tiles (a ragged batch of ~1000 live rows x a 512- or 1024-wide output: 136-272 live tiles on
      // 256 CUs): 32-row tiles double the work-groups.  Measured at configs[2] (M3_TILED_THIN_BELOW=600): one context alone
      // 3.94 -> 3.72 ms, four contexts 2.42 -> 2.31 M frames/s (W tiles are fetched twice as often) -- a latency / throughput
      // trade, off by default.  (k-steps of 256 with one work-group per CU were tried for launches of <= 256 tiles: half the
      // round trips, but 13.2 vs 9.0 us at 1090 x 1024 x 512 and 4.39 vs 3.95 ms per configs[2] forward -- two resident
      // work-groups that overlap each other's waits are worth more than fewer, longer steps)
      const bool thin = !big && !conv && (long)cdiv(p.M, 64) * cdiv(p.N, 64) < thin_below;
      if (big) tiled_grid(p, plan, 128, 128, 64); else tiled_grid(p, plan, thin ? 32 : 64, 64, 128);
      return true;
    }
    M3_PLAN_REQUIRE(!p.a_bf16 && !p.y_bf16 && p.Yb == nullptr, "%s: bf16 activations are a feature of the tiled kernel", who);
    plan.kernel = GemmKernel::SkinnyBf16; plan.label = "gemm_bf16w_kernel";
    skinny_grid(p, plan, Nout);
    return true;
  }
  const char* who = "gemm";
  if (concat) M3_PLAN_REQUIRE((p.K1 & 15) == 0 && p.A2 != nullptr && (p.lda2 & 3) == 0, "%s: bad concat operands", who);
  M3_PLAN_REQUIRE(!(p.ln_wsum && p.ln_gamma), "%s: folded (ln_wsum) and affine (ln_gamma) LayerNorm are exclusive", who);
  if (plan.ln != GEMM_LN_NONE) {
    M3_PLAN_REQUIRE(p.mode == GEMM_A_PLAIN || (concat && p.ln_on_a2), "%s: LayerNorm needs plain A (or the A2 half of a concat)", who);
    M3_PLAN_REQUIRE((p.ln_on_a2 ? p.K - p.K1 : p.K) <= 1024, "%s: LayerNorm supports rows up to 1024 wide", who);
    M3_PLAN_REQUIRE(p.K <= 2047, "%s: LayerNorm variants are built for K < 2048", who);
  }
  M3_PLAN_REQUIRE(!p.ln_on_a2 || concat, "%s: ln_on_a2 needs concat mode", who);
  M3_PLAN_REQUIRE(p.ln_out == nullptr || plan.ln == GEMM_LN_PRO, "%s: ln_out needs the affine LayerNorm prologue", who);
  if (long_batch && (p.K & 63) == 0 && (!conv || (p.conv_C & 63) == 0)) {
    plan.kernel = GemmKernel::TiledF32; plan.label = "gemm_f32_tiled_kernel";
    if (big) tiled_grid(p, plan, 128, 128, 32); else tiled_grid(p, plan, 64, 64, 64);
    return true;
  }
  plan.kernel = GemmKernel::SkinnyF32; plan.label = "gemm_f32_kernel";
  skinny_grid(p, plan, Nout);
  // the dual instantiations: 16-row tiles, 4 / 8 waves, one load group per wave (every block GEMM of the model at B = 1)
  plan.dual_ok = plan.mt == 1 && (plan.nw == 4 || plan.nw == 8) && plan.nbuf == 1 && p.mode == GEMM_A_PLAIN &&
                 plan.ln != GEMM_LN_PRO && p.m_dev == nullptr && p.acc_init == nullptr;
  return true;
}

// sig_col0 and acc_init are features of the skinny fp32 kernel alone (kernels.h says of which of its forms)
static bool extras_ok(const GemmParams& p, GemmPlan& plan) {
  if (p.sig_col0 >= 0) {
    M3_PLAN_REQUIRE(plan.kernel == GemmKernel::SkinnyF32 && !plan.glu, "gemm: sig_col0 needs the skinny fp32 kernel with a plain epilogue (M=%d N=%d K=%d)",
                    p.M, p.N, p.K);
    M3_PLAN_REQUIRE((p.sig_col0 & 15) == 0, "gemm: sig_col0=%d must be a multiple of 16", p.sig_col0);
  }
  if (p.acc_init != nullptr) {
    M3_PLAN_REQUIRE(plan.kernel == GemmKernel::SkinnyF32 && plan.mt == 1 && !plan.glu && p.mode == GEMM_A_CONCAT2 && (p.K1 & 15) == 0,
                    "gemm: acc_init needs the skinny fp32 kernel, 16-row tiles, concat operands with K1 %% 16 == 0");
    M3_PLAN_REQUIRE(plan.ln == GEMM_LN_PRO && p.ln_on_a2 && (plan.nw == 4 || plan.nw == 8) && plan.nbuf == 1 && 2 * p.K1 == p.K &&
                    p.K == 16 * plan.nw * gemm_group_steps(1, 1, plan.nw),
                    "gemm: acc_init is built for K1 = K / 2 = %d with the LayerNorm prologue on the A2 half (K1=%d K=%d)",
                    8 * plan.nw * gemm_group_steps(1, 1, plan.nw), p.K1, p.K);
  }
  if (p.w_frag) {   // fragment-ordered W: only gemm_f32_body's load_group knows the layout
    M3_PLAN_REQUIRE(!p.w_bf16, "gemm: fragment-ordered weights are fp32-only");
    M3_PLAN_REQUIRE(p.mode == GEMM_A_PLAIN, "gemm: fragment-ordered weights need plain A (no concat, no implicit conv)");
    const int Nout = plan.glu ? p.N / 2 : p.N;
    M3_PLAN_REQUIRE((Nout & 15) == 0 && (p.K & 15) == 0, "gemm: fragment-ordered weights need N%s=%d and K=%d to be multiples of 16",
                    plan.glu ? " / 2" : "", Nout, p.K);
    M3_PLAN_REQUIRE(plan.kernel == GemmKernel::SkinnyF32, "gemm: fragment-ordered weights need the skinny fp32 kernel; M=%d N=%d K=%d plans as %s",
                    p.M, p.N, p.K, plan.label);
  }
  return true;
}

GemmPlan plan_gemm(const GemmParams& p, size_t workspace_bytes_available) {
  GemmPlan plan{};
  plan.kernel = p.w_bf16 ? GemmKernel::SkinnyBf16 : GemmKernel::SkinnyF32;
  plan.label = "";
  plan.glu = p.act == ACT_GLU; plan.conv = p.mode == GEMM_A_CONV3X3S2;
  plan.ln = p.ln_wsum ? GEMM_LN_EPI : (p.ln_gamma ? GEMM_LN_PRO : GEMM_LN_NONE);
  if (operands_ok(p, p.w_bf16 ? "gemm_bf16w" : "gemm", plan) && choose_form(p, workspace_bytes_available, plan) && extras_ok(p, plan))
    plan.launches = plan.kernel == GemmKernel::SplitKF32 ? 2 : 1;
  return plan;
}

GemmLaunch gemm_launch(const GemmParams& p, float* ws, size_t ws_bytes) { return GemmLaunch{p, plan_gemm(p, ws != nullptr ? ws_bytes : 0), ws}; }
bool gemm_dual_fusable(const GemmLaunch& ga, const GemmLaunch& gb) {
  const GemmPlan &a = ga.plan, &b = gb.plan;
  return a.launches == 1 && b.launches == 1 && a.dual_ok && b.dual_ok && a.nw == b.nw && a.ln == b.ln && a.glu == b.glu &&
         !ga.p.w_frag == !gb.p.w_frag;
}

int launch_gemm(const GemmLaunch& g, hipStream_t stream) {
  const GemmPlan& plan = g.plan; const GemmParams& p = g.p; float* const ws = g.ws;
  M3_REQUIRE(plan.launches > 0, "%s", plan.reason);
  switch (plan.kernel) {
    case GemmKernel::SkinnyF32: return launch_gemm_f32_skinny(plan, p, stream);
    case GemmKernel::SkinnyBf16: return launch_gemm_bf16w_skinny(plan, p, stream);
    case GemmKernel::TiledF32: return launch_gemm_f32_tiled(plan, p, stream);
    case GemmKernel::TiledBf16: return launch_gemm_bf16w_tiled(plan, p, stream);
    case GemmKernel::DmaBf16: return launch_gemm_bf16_dma(plan, p, stream);
    case GemmKernel::SplitKF32:
      M3_REQUIRE(ws != nullptr, "gemm split-K: the plan was made for a workspace of %zu bytes, none given", plan.ws_bytes);
      return launch_gemm_f32_splitk(plan, p, ws, stream);
  }
  return -2;
}

}  // namespace m3
