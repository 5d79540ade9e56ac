// Internal launcher interface of libm3asr_hip.so (C++ side; the C-ABI lives in include/m3asr.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/m3asr.h"

namespace m3 {

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SILU = 2, ACT_GLU = 3 };
enum { GEMM_A_PLAIN = 0, GEMM_A_CONCAT2 = 1, GEMM_A_CONV3X3S2 = 2 };

// x / d for 0 <= x < 2^31 as (x * mul) >> shift in 64 bits, exact: shift = 31 + l with l = ceil(log2 d), mul = ceil(2^shift / d)
// < 2^32 (Granlund & Montgomery, "Division by invariant integers using multiplication", 1994, theorem 4.2 with N = 31:
// 2^shift <= mul * d <= 2^shift + 2^l).  On the device two multiplications and a shift instead of a ~30-instruction sequence.
struct GemmDiv { unsigned mul = 0; int shift = 0; };
inline GemmDiv gemm_div(int d) {
  int l = 0;
  while (l < 31 && (1u << l) < (unsigned)d) ++l;
  GemmDiv r;
  r.shift = 31 + l;
  r.mul = (unsigned)(((1ull << r.shift) + (unsigned)d - 1) / (unsigned)d);
  return r;
}

struct GemmParams {
  // operands: Y[M,Nout] = epi( pro(A)[M,K] . W[N,K]^T )
  const float* A = nullptr; int lda = 0;
  const float* A2 = nullptr; int lda2 = 0; int K1 = 0;   // CONCAT2: k<K1 from A, else A2[k-K1]
  const float* W = nullptr;                               // [N][K] row-major (fp32, or bf16 when w_bf16)
  int w_bf16 = 0;                                         // W holds bf16: operands rounded at the MFMA input, fp32 accumulate
  const float* bias = nullptr;                            // [N] or null
  float* Y = nullptr; int ldy = 0;
  int M = 0, N = 0, K = 0;
  int mode = GEMM_A_PLAIN;
  // prologue
  const float* ln_gamma = nullptr; const float* ln_beta = nullptr; float ln_eps = 0.f;
  // folded LayerNorm (affine already inside W / bias): wsum[n] = sum_k W'[n][k]; wbeta[n] = (W . beta)[n] (only with mask_in)
  const float* ln_wsum = nullptr; const float* ln_wbeta = nullptr;
  int ln_on_a2 = 0;                                       // CONCAT2: LayerNorm only the A2 half (router input)
  float* ln_out = nullptr; int ld_ln_out = 0;             // optional side output of the normalised rows
  const int32_t* row_len = nullptr; int rows_per_batch = 0;  // frame t = row % rows_per_batch is padded if t >= row_len[row / rows_per_batch]
  int mask_in = 0, mask_out = 0;
  // implicit 3x3 stride-2 conv over a channel-last (B,T1,F1,C) input -> rows (b,t2,f2)
  int conv_T1 = 0, conv_F1 = 0, conv_T2 = 0, conv_F2 = 0, conv_C = 0;
  // epilogue
  int act = ACT_NONE;
  float alpha = 1.f;
  const float* resid = nullptr; int ldr = 0;
  // grouped (per-expert) form of the tiled bf16 kernel: row tiles cut from acc_hist, optional row gather, slice-major W
  const int32_t* grp_acc = nullptr; int grp_E = 0; const int32_t* grp_pos = nullptr; int w_sliced = 0;
  const float* w_scale = nullptr;                         // fp8 weights (grouped forms): per-output-row scale [E][N]; MXFP4 weights: the
                                                          // e8m0 scale BYTES, [E][N][K/32] or slice-major [E][K/64][N][2] (w_sliced)
  // bf16 activation copies (16-bit modes, tiled kernel only): A given as bf16 [M][lda], Y written as bf16, and / or an
  // additional bf16 copy Yb of the fp32 output (the residual stream stays fp32, its GEMM consumers read the copy)
  int a_bf16 = 0, y_bf16 = 0; void* Yb = nullptr; int ldyb = 0;
  // Row statistics of a bf16 operand for the folded LayerNorm of its consumer (gemm_bf16_dma.hip, where nothing passes
  // through registers while staging): per row kXbStatParts partial (sum, sum of squares) pairs of the bf16 values.
  // Yb_stats: the kernel that writes Yb also writes its column tile's partial; ln_stats: the LayerNorm GEMM reads them
  float* Yb_stats = nullptr; const float* ln_stats = nullptr; int ln_stat_parts = 0;
  // packed ragged batches: device-side count of live rows; work-groups whose first row lies beyond it exit (the row AT
  // the count is still computed: it carries the conv module's pad-frame constant, see dwconv_ln_silu_kernel)
  const int32_t* m_dev = nullptr;
  const int32_t* y_rows = nullptr;                        // grouped GEMM-2 only: output row m goes to row y_rows[m] of Y (expert-parallel: straight to its wire row)
  // implicit conv on a packed ragged batch: valid output frames per utterance; a tile whose rows (b, t2, f2) all lie past
  // the utterance's last frame is skipped (its output rows are never gathered into the packed layout)
  const int32_t* conv_len = nullptr;
  // skinny fp32 kernel, plain epilogue: output columns >= sig_col0 (a multiple of 16; -1: none) are stored as sigmoid(y) -- the
  // GLU gate of a deferred-GLU pointwise_conv1, sigmoided once where the epilogue holds it instead of once per depthwise tap
  int sig_col0 = -1;
  // skinny fp32 kernel, 16-row tiles, concat mode with K1 == K / 2 and one load group per wave: the accumulator pair every wave
  // holds after its A-half K-steps, [m_tile][n_tile][wave][2][64 lanes] float4, as router_embed_prefix_kernel leaves it.  The wave
  // starts from it and runs its A2-half steps only (an MFMA chain cut and resumed from the stored registers: the same bits)
  const float* acc_init = nullptr;
  // skinny fp32 kernel, plain A, N (GLU: N / 2) and K multiples of 16: W is in MFMA-fragment order (include/m3asr.h "fragment
  // order"), Wf[N/16][K/16][4 (kq)][16 (col)][4] -- lane 16 * kq + col reads bytes [16 * lane, 16 * lane + 16) of the KB of
  // (column tile, K-step), so one wave load instruction is one contiguous KB.  Every lane receives the same 16 bytes as from
  // the row-major matrix: same bits.  plan_gemm refuses it everywhere else.
  int w_frag = 0;
  // filled by the launchers from the GemmPlan
  int n_tiles = 0, m_tiles = 0, xcd_swizzle = 0;
  // skinny fp32 kernel only (gemm_fill_tiles, gemm.hip).  one_run: rows_per_batch >= M, so every row belongs to utterance 0 and its
  // frame is its row (B = 1, and a packed batch whose rows_per_batch is its row count): the masks need no division at all.
  // div_m_tiles / div_n_tiles / div_rpb: the divisors of the tile order and of the masks as multiplications (GemmDiv)
  int one_run = 0;
  GemmDiv div_m_tiles, div_n_tiles, div_rpb;
};
// ---- the dense GEMM family (gemm_plan.hip) ----
// The family has six kernels.  plan_gemm is the ONE place that checks a problem's operands and says which kernel runs it, in
// which instantiation, over which grid and with how much workspace.  One launch is one record, GemmLaunch: the problem, its plan and
// the workspace the plan was made against (gemm_launch).  launch_gemm runs a record, the pair launchers and *_dual_fusable read two; the
// engine's stage list, its workspace sizing and the observability entries (m3_linear_kernel, m3_engine_stage_info) read the same plan.  First match wins:
//   SplitKF32   fp32 W, K >= 4096, K % 64 == 0, N, lda, ldy % 4 == 0, at most 160 tiles of 64 x 64, plain epilogue (bias /
//               ReLU / SiLU / scale), >= 2 K ranges of >= 4 k-steps, and the caller's workspace holds them      2 launches
//   DmaBf16     bf16 W and bf16 A, M >= 4096 (M3_DMA_MIN_ROWS), plain A, K % 64 == 0, lda % 8 == 0, operands < 4 GB,
//               folded LayerNorm only with ln_stats                                                             1 launch
//   TiledBf16   bf16 W, M >= 384 (M3_TILED_MIN_ROWS), >= 160 tiles of 64 x 64, K (conv: C) % 128 == 0          1 launch
//   TiledF32    fp32 W, the same row and tile bounds, K (conv: C) % 64 == 0, no concat, no affine LayerNorm    1 launch
//   SkinnyBf16  bf16 W, fp32 A and Y, no Yb                                                                     1 launch
//   SkinnyF32   fp32 W, everything else                                                                         1 launch
// Yb_stats / ln_stats exist on DmaBf16 only; concat operands and the affine LayerNorm on SkinnyF32 only.  A problem no row
// takes comes back with launches = 0 and the reason as text.  The thresholds are read once per process.
enum { GEMM_LN_NONE = 0, GEMM_LN_EPI = 1, GEMM_LN_PRO = 2 };   // none / folded, applied in the epilogue (ln_wsum) / affine prologue (ln_gamma)
enum class GemmKernel { SkinnyF32, SkinnyBf16, TiledF32, TiledBf16, DmaBf16, SplitKF32 };
struct GemmPlan {
  GemmKernel kernel;
  const char* label;      // the kernel's name as rocprofv3 shows it
  int launches;           // 1, 2 for split-K (+ its reduce), 0: a problem the family does not take (reason says why)
  bool glu, conv; int ln; // template arguments every kernel shares (GEMM_LN_*)
  int mt, nw, nbuf;       // skinny kernels: 16 * mt rows per work-group, K split over nw waves, one / two staging buffers
  bool dual_ok;           // SkinnyF32 in one of the instantiations gemm_f32_dual_kernel has (gemm_dual_fusable)
  int bm, bn, bk;         // tiled kernels: the tile
  int stages;             // DmaBf16: depth of the LDS ring
  int m_tiles, n_tiles, xcd_swizzle;   // what the launcher puts into the kernel's GemmParams; the grid follows from them
  int splits; size_t ws_bytes;         // SplitKF32: K ranges and the partial tiles they leave in the workspace
  char reason[192];
};
GemmPlan plan_gemm(const GemmParams& p, size_t workspace_bytes_available);
struct GemmLaunch { GemmParams p; GemmPlan plan; float* ws = nullptr; };
GemmLaunch gemm_launch(const GemmParams& p, float* ws, size_t ws_bytes);   // p planned against ws (a null ws: against 0 bytes)
int launch_gemm(const GemmLaunch& g, hipStream_t stream);
bool gemm_dual_fusable(const GemmLaunch& a, const GemmLaunch& b);   // two independent skinny fp32 GEMMs of one instantiation
int launch_gemm_f32_dual(const GemmLaunch& a, const GemmLaunch& b, hipStream_t stream);   // ... in ONE launch
// The A (embed) half of up to kRouterPrefixMaxLayers concat GEMMs that share A, M, N, K, K1 and differ in W: the accumulator
// pairs GemmParams::acc_init takes, layer l's at prefix + l * router_prefix_floats(plan).  `plan`: the consumers' plan (a form
// that takes acc_init); layers [layer0, layer0 + n_layers) of w[] are computed, one launch.
constexpr int kRouterPrefixMaxLayers = 64;
size_t router_prefix_floats(const GemmPlan& plan);   // per layer
int launch_router_embed_prefix(const GemmPlan& plan, const GemmParams& p, const float* const* w, int layer0, int n_layers, float* prefix,
                               hipStream_t stream);
// K-steps per in-flight load group of the skinny kernels (the planner needs them for nbuf).  fp32: 2 buffers x G x (NT + MT)
// float4 must fit the per-lane register budget (512 VGPR+AGPR for 4 waves, 256 for 8, 128 for 16 waves per workgroup)
constexpr int gemm_group_steps(int MT, int NT, int NW) {
  if (NW == 16) return MT == 1 ? (NT == 1 ? 4 : 2) : (MT == 2 ? 2 : 1);
  if (NW == 8) return MT == 1 ? 8 : (MT == 2 ? (NT == 1 ? 6 : 4) : (NT == 1 ? 3 : 2));
  return MT == 1 ? 8 : (MT == 2 ? 6 : 4);
}
constexpr int gemm16_group_steps(int MT, int NW) { return NW == 16 ? 2 : (MT == 4 ? 2 : 4); }
// The per-form launchers launch exactly one form each, in the plan's instantiation: no decision, no operand check.
int launch_gemm_f32_skinny(const GemmPlan& plan, const GemmParams& p, hipStream_t stream);      // gemm.hip
int launch_gemm_bf16w_skinny(const GemmPlan& plan, const GemmParams& p, hipStream_t stream);    // gemm_bf16.hip
int launch_gemm_f32_tiled(const GemmPlan& plan, const GemmParams& p, hipStream_t stream);       // gemm_f32_tiled.hip
int launch_gemm_bf16w_tiled(const GemmPlan& plan, const GemmParams& p, hipStream_t stream);     // gemm_bf16_tiled.hip
// bf16 A x bf16 W, LDS-DMA fed 128 x 128 x 64 tiles: the dense GEMMs of long batches in the 16-bit modes
int launch_gemm_bf16_dma(const GemmPlan& plan, const GemmParams& p, hipStream_t stream);        // gemm_bf16_dma.hip
// deep-K, few-tile fp32 problems (conv2 / subsampling Linear at short inputs): split-K tiled kernel + reduce
int launch_gemm_f32_splitk(const GemmPlan& plan, const GemmParams& p, float* ws, hipStream_t stream);   // gemm_f32_splitk.hip
// two independent split-K problems (both implicit convs or both plain), each with its own workspace, in one GEMM + one reduce launch
bool gemm_splitk_dual_fusable(const GemmLaunch& a, const GemmLaunch& b);
int launch_gemm_f32_splitk_dual(const GemmLaunch& a, const GemmLaunch& b, hipStream_t stream, int which = 3);   // which: 1 the GEMM launch, 2 the reduce launch, 3 both
// once, outside graph capture (dynamic-LDS opt-in of the tiled kernels)
int init_gemm_f32_splitk_kernels();
int init_gemm_bf16_tiled_kernels();
int init_gemm_f32_tiled_kernels();
int init_gemm_bf16_dma_kernels();
constexpr int kXbStatParts = 4;                          // partial row statistics kept per row of a bf16 activation copy
// (sum, sum of squares) of every row of a bf16 matrix -> stats[row][kXbStatParts][2] (total in part 0, zeros elsewhere)
int launch_row_stats_bf16(const void* xb, int rows, int D, float* stats, hipStream_t stream);

// ---- MoE indexing / scatter / gather (moe_index.hip) ----
int launch_moe_index(const int32_t* gate_idx, int S, int E, int32_t* mapping, int32_t* acc_hist,
                     int32_t* pos, hipStream_t stream);
// SoftmaxTopK + ScatterMapping fused (router logits [S][width] -> gate_idx, gate_value, mapping, acc, pos)
int launch_moe_gate_index(const float* logits, int width, const int32_t* row_len, int rows_per_batch, int S,
                          int32_t* gate_idx, float* gate_value, int32_t* mapping, int32_t* acc_hist, int32_t* pos,
                          hipStream_t stream);
// router (x half, folded LayerNorm) + softmax-top1 + index in one single-workgroup launch (S <= 256)
int launch_moe_route(const float* x, int ldx, int D, const float* wx, const float* wsum, const float* bias,
                     const float* eall, int ld_e, float ln_eps, const int32_t* row_len, int rows_per_batch, int S, int E,
                     int32_t* gate_idx, float* gate_value, int32_t* mapping, int32_t* acc_hist, int32_t* pos,
                     hipStream_t stream);
// router product on cat([embed, LayerNorm(x)]) with the normalised rows written out (moe_router.hip): one work-group per 16
// rows and all N <= 64 experts
bool moe_router_supports(int De, int D, int N);
bool moe_router_fuses_top1(int N);   // SoftmaxTopK in the router kernel's tail (gate_idx / gate_val arguments of launch_moe_router)
int init_moe_router_kernels();
int launch_moe_router(const float* emb, int lde, int De, const float* x, int ldx, int D, const float* W, const float* bias,
                      const float* gamma, const float* beta, float eps, float* xn, int ldxn, float* Y, int ldy, int M, int N,
                      const int32_t* m_dev, hipStream_t stream, int32_t* gate_idx = nullptr, float* gate_val = nullptr,
                      const int32_t* row_len = nullptr, int rows_per_batch = 0, void* xq = nullptr, float* xq_scale = nullptr);
int launch_local_scatter(const void* x, const int32_t* mapping, int S, int row_bytes, void* out, hipStream_t stream);
int launch_local_gather(const void* buf, const int32_t* mapping, int S, int row_bytes, void* out, hipStream_t stream);

// ---- expert-parallel exchange bookkeeping on the device (ep_exchange.hip) ----
int launch_ep_send_map(const int32_t* gate_idx, const int32_t* mapping, const int32_t* acc_hist, int S, int world, int e_loc,
                       int capacity, int32_t* map_send, void* wire, int row_bytes, hipStream_t stream, int32_t* overflow = nullptr);
int launch_ep_send_rows(const int32_t* gate_idx, const int32_t* mapping, const int32_t* acc_hist, int S, int world, int e_loc,
                        int capacity, int32_t* map_send, const void* x, void* wire, int row_bytes, hipStream_t stream, int32_t* overflow = nullptr);   // send map + scatter, one launch
int launch_ep_recv_gate(const void* wire, int world, int e_loc, int capacity, int row_bytes, int32_t* gate_recv,
                        hipStream_t stream);

// ---- grouped expert FFN (moe_expert.hip) ----
#ifndef M3_EXPERT_SLICE
#define M3_EXPERT_SLICE 64        // (16 / 32: experiment builds next to the tree, tools/exp_ffn_pair.py; the plan format assumes 64)
#endif
constexpr int kExpertSliceW16 = 64;            // the bf16 / e4m3 slab kernels are laid out for 64-wide slices
constexpr int kExpertSlice = M3_EXPERT_SLICE;  // hidden units per workgroup (16 per wave); m3asr/plan.py EXPERT_SLICE must match
size_t expert_ffn_slab_bytes(int S, int D, int F);   // the slab region: F / kExpertSlice partial-result slabs of [S][D] fp32
// The operator runs in ten forms.  plan_expert_ffn (moe_expert_plan.hip) is the ONE place that says which of them runs for a
// weight dtype and shape, in how many launches, and where in the slab region its sections are; launch_expert_ffn runs a plan,
// and the combine step, the launch accounting and the observability entries read the same plan.  First match wins:
//   FusedFp8   FP8A8, D = 512, F % 128 == 0, F <= 4096, E <= 1024, S >= 4096 (M3_EXPERT_FUSED_FP8_MIN_ROWS), S >= 64 E,
//              and an F split exists (expert_ffn_fused_fp8_fsplit)          1 launch,   fsplit slabs of sorted rows at offset 0
//   G256Bf16   BF16, a TiledBf16 shape with E <= 64, S / E >= 512 (M3_G256_MIN_ROWS_PER_EXPERT), D, F % 256 == 0,
//              not EXPERT_SCATTER_ROWS                                      3 launches, H | sorted rows | bf16 row copy
//   Tiled*     S >= 1024 (M3_EXPERT_TILED_MIN_ROWS), D, F % 64 == 0 (fp32) or % 128 == 0 (bf16, fp8, mxfp4; FP8A8 where the
//              fused form does not apply), not EXPERT_NORM_IN_KERNEL        2 launches, H | sorted rows (one slab)
//   Slab*      everything else: D % 16 == 0 (fp32), % 32 (bf16), % 64 (fp8), % 128 (mxfp4: SlabW4), D <= 2048, F % 64 == 0
//                                                                           1 launch,   F / 64 partial-result slabs at offset 0
// A form is taken only if all its sections fit into expert_ffn_slab_bytes.  The thresholds are read once per process.
// (SlabF32's weight stream keeps the default cache policy also where every byte has one reader: non-temporal loads there lost)
enum class ExpertWeights { F32, BF16, FP8, FP8A8, MXFP4 };   // FP8A8: fp8 weights + fp8 activations where FusedFp8 applies, else the weight-only forms
enum class ExpertKernel { SlabF32, TiledF32, SlabBf16, TiledBf16, G256Bf16, SlabW8, TiledW8, FusedFp8, SlabW4, TiledW4 };
struct ExpertFfnPlan {
  ExpertWeights weights; ExpertKernel kernel;
  const char* label;      // the kernel's name as rocprofv3 shows it
  int launches, slices;   // kernel launches (0: dimensions no form takes, the launcher says which); partial-result slabs the combine sums
  int fsplit;             // FusedFp8 only
  size_t h_off, rows_off, xb_off;   // byte offsets inside the slab region (0 where unused): H, the result rows / slabs, the bf16 row copy
  float* rows(float* slab) const { return (float*)((char*)slab + rows_off); }   // what moe_combine reads
};
enum { EXPERT_NORM_IN_KERNEL = 1,    // norm_ff applied while gathering rows: fp32 slab form only
       EXPERT_SCATTER_ROWS = 2 };    // GEMM-2 writes b2 + rows to y_scatter[pos[i]]: bf16 tiled form only, never g256
ExpertFfnPlan plan_expert_ffn(ExpertWeights w, int S, int E, int D, int F, unsigned flags = 0);
// x [S][ldx] fp32 rows, sorted by expert through (pos, acc_hist); w1 [E][F][D], w2 [E][D][F] or slice-major (w2_sliced) in the
// plan's weight dtype; s1 [E][F] / s2 [E][D]: fp8 per-row scales.  MXFP4: w1 [E][F][D/2], w2 [E][D][F/2] or slice-major
// [E][F/64][D][32] code bytes, s1 / s2 carry the e8m0 scale BYTES ([E][F][D/32]; [E][D][F/32] or [E][F/64][D][2]).  ln_*: SlabF32 under EXPERT_NORM_IN_KERNEL.  h_scale, xq /
// xq_scale (rows already quantised by the router kernel), fs_dev (the kernel may split F finer than the plan and leaves the
// slab count there): FusedFp8.  b2 / y_scatter: TiledBf16 under EXPERT_SCATTER_ROWS (the un-permute of the expert-parallel
// receive side, folded into GEMM-2's epilogue).
// w2_sliced, as the launchers take it: EXPERT_W_FRAG -- w1 AND w2 in MFMA-fragment order (pack_wfrag of w1 and of the slice-major w2;
// include/m3asr.h "fragment order") -- is read by expert_ffn_f32_kernel alone: the SlabF32 form and the self-routing launch
enum { EXPERT_W_REF = 0, EXPERT_W2_SLICED = 1, EXPERT_W_FRAG = 2 };
struct ExpertFfnArgs { const float* x; int ldx; const int32_t *pos, *acc_hist; const void *w1, *w2; const float *s1, *s2, *b1, *b2;
                       int w2_sliced; float h_scale; float* slab; const float *ln_gamma, *ln_beta; float ln_eps;
                       const void* xq; const float* xq_scale; int32_t* fs_dev; float* y_scatter; };
int launch_expert_ffn(const ExpertFfnPlan& plan, int S, int E, int D, int F, const ExpertFfnArgs& a, hipStream_t stream);
// The per-form launchers below launch exactly one form each (their own argument checks and tile sizes, no decision about form).
int init_expert_ffn_kernels();
int launch_expert_ffn_f32_slab(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E,
                               int D, int F, const float* w1, const float* b1, const float* w2, int w2_sliced, float* slab,
                               const float* ln_gamma, const float* ln_beta, float ln_eps, hipStream_t stream);
// long batches: two grouped LDS-tiled fp32 GEMMs (moe_expert_tiled_f32.hip); hbuf S*F fp32, ybuf S*D fp32
int init_expert_ffn_f32_tiled_kernels();
int launch_expert_tiled_f32(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E,
                            int D, int F, const float* w1, const float* b1, const float* w2, int w2_sliced,
                            float* hbuf, float* ybuf, hipStream_t stream);
// bf16 weights (w1 [E][F][D], w2 as above), fp32 rows in / fp32 slab out (moe_expert_bf16.hip)
int init_expert_ffn_bf16_kernels();
int launch_expert_ffn_bf16w_slab(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E,
                                 int D, int F, const void* w1, const float* b1, const void* w2, int w2_sliced, float* slab,
                                 hipStream_t stream);
// fp8 (e4m3) expert weights + per-row scales, dequantised to bf16 at the MFMA input (moe_expert_fp8.hip); same result layout as bf16
int init_expert_ffn_w8_kernels();
int launch_expert_ffn_w8_slab(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E, int D, int F,
                              const void* w1, const float* s1, const float* b1, const void* w2, const float* s2, int w2_sliced,
                              float* slab, hipStream_t stream);
// MXFP4 expert weights (e2m1 code pairs + e8m0 block scales), decoded to bf16 at the MFMA input (moe_expert_mxfp4.hip); same result layout
int init_expert_ffn_w4_kernels();
int launch_expert_ffn_w4_slab(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E, int D, int F,
                              const void* w1, const void* s1, const float* b1, const void* w2, const void* s2, int w2_sliced,
                              float* slab, hipStream_t stream);
// fp8 arithmetic (e4m3 weights x e4m3 activations, fp8 MFMA), long batches (D = 512): moe_expert_fused_fp8.hip.
// The F split its cost model picks for a shape the kernel takes, 0 where it does not apply (the row threshold is the plan's)
constexpr int kExpertFusedFp8MaxSplit = 4;     // ... at most this (what the combine allots when the kernel picks the split on the device)
int expert_ffn_fused_fp8_fsplit(int S, int E, int D, int F);
int init_expert_ffn_fused_fp8_kernels();
int launch_expert_ffn_fused_fp8(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E, int D, int F,
                                const void* w1, const float* s1, const float* b1, const void* w2, const float* s2, int w2_sliced,
                                float h_scale, int fsplit, float* ybuf, hipStream_t stream, const void* xq = nullptr,
                                const float* xq_scale = nullptr, int32_t* fs_dev = nullptr);
int launch_quantize_rows_e4m3(const float* x, int ldx, int S, int D, void* xq, float* scale, hipStream_t stream);   // moe_expert_fused_fp8.hip
// long batches, bf16, fp8 (w_fp8 = 1: s1 / s2 per-row scales) or MXFP4 (w_fp8 = 2: s1 / s2 the scale bytes) weights: two grouped GEMMs
// on the LDS-tiled bf16 core (gemm_bf16_tiled.hip); hbuf S*F bf16, ybuf S*D fp32.  b2 / y_scatter (optional, bf16 weights): GEMM-2 adds the expert's b2
// and writes row i of the sorted order to row pos[i] of y_scatter
int launch_expert_tiled_w16(int w_fp8, const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E,
                            int D, int F, const void* w1, const float* s1, const float* b1, const void* w2, const float* s2,
                            int w2_sliced, void* hbuf, float* ybuf, hipStream_t stream, const float* b2 = nullptr,
                            float* y_scatter = nullptr);
// SoftmaxTopK + ScatterMapping + grouped expert FFN in ONE launch (S <= 256 rows, all experts local, fp32): see moe_expert.hip
bool expert_ffn_f32_self_routing(int S, int E);
int launch_expert_route_ffn_f32(const float* x, int ldx, const float* logits, const int32_t* row_len, int rows_per_batch, int S, int E,
                                int D, int F, const float* w1, const float* b1, const float* w2, int w2_sliced, const float* b2,
                                float* slab, int32_t* gate_idx, float* gate_value, int32_t* mapping, int32_t* acc_hist, int32_t* pos,
                                hipStream_t stream, const float* ln_gamma = nullptr, const float* ln_beta = nullptr, float ln_eps = 0.f);
// grouped bf16 expert GEMMs on 256 x 256 x 64 LDS-DMA tiles (expert_gemm_g256.hip): saturating row counts (>= 512 rows per expert).
// xb: bf16 copy of the rows (launch_rows_to_bf16), S*D bf16
bool expert_gemm_g256_takes(int S, int E, int D, int F);   // what the kernel can run at all (not whether it pays: the plan)
int init_expert_gemm_g256_kernels();
int launch_rows_to_bf16(const float* x, int ldx, int S, int D, void* xb, hipStream_t stream);
int launch_expert_ffn_bf16_g256(const void* xb, int ldxb, const int32_t* pos, const int32_t* acc_hist, int S, int E, int D, int F,
                                const void* w1, const float* b1, const void* w2, int w2_sliced, void* hbuf, float* ybuf,
                                hipStream_t stream);
// out[s] = resid[s] + alpha * gate[s] * (b2[g_s] + sum_slices slab[slice][mapping[s]]), optional LayerNorm after
int launch_moe_combine(const float* slab, int n_slices, const int32_t* mapping, const int32_t* gate_idx,
                       const float* gate_value, const float* b2, const float* resid, float alpha,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, float* out, int S, int D,
                       hipStream_t stream, void* out_bf16 = nullptr, float* out_stats = nullptr,
                       const int32_t* n_slices_dev = nullptr);   // n_slices_dev: the slab count is a device value (<= n_slices)

// ---- row-wise ops (rowops.hip) ----
int launch_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int D,
                     hipStream_t stream, void* y_bf16 = nullptr, float* y_stats = nullptr, const float* gamma2 = nullptr,
                     const float* beta2 = nullptr, float eps2 = 0.f, float* y2 = nullptr);   // gamma2: y2 = LN2(LN1(x)) in the same launch
int launch_softmax_top1(const float* logits, int ld, const int32_t* row_len, int rows_per_batch, int S, int E,
                        int32_t* idx, float* value, hipStream_t stream);
int launch_att_masked_softmax(const float* scores, const int32_t* len, int B, int H, int T1, int T2, float scale,
                              float* out, hipStream_t stream);
int launch_masked_fill(const float* x, const int32_t* len, int B, int C, int T, float fill, float* y,
                       hipStream_t stream);
int launch_glu(const float* x, int outer, int C, int inner, float* y, hipStream_t stream);
int launch_scale(const float* x, float scale, float* y, size_t n, hipStream_t stream);
int launch_mask_conv2d_sample(const int32_t* len_in, int B, int left_padding, int stride, int32_t* len_out,
                              hipStream_t stream);
int launch_subsample_lens(const int32_t* len_in, int B, int32_t* len_out, hipStream_t stream);
int launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t stream);
int launch_binary_bcast(const float* a, const float* b, float* y, const int64_t* shape, const int64_t* sa,
                        const int64_t* sb, int nd, int op, hipStream_t stream);
int launch_unary(const float* x, float* y, size_t n, int act, hipStream_t stream);
int launch_permute(const float* x, float* y, const int64_t* out_shape, const int64_t* in_strides, int nd,
                   hipStream_t stream);
int launch_concat_last(const float* a, int da, const float* b, int db, float* y, size_t rows, hipStream_t stream);
int launch_softmax_lastdim(const float* x, float* y, size_t rows, int n, hipStream_t stream);
int launch_bmm(const float* a, const float* b, float* c, int batch, int M, int N, int K, int64_t sa, int64_t sb,
               int trans_b, hipStream_t stream);

// ---- fused rel-pos attention (attention.hip) ----
// One record per problem (what the engine keeps per stage and the C ABI fills from its descriptor), one check, one launcher for the
// three cores; two fp32 problems with head widths 64 or 128 each can share a launch.
//   fp32 rows (default): qkv fp32 [B*T][ldq], out fp32 (or bf16 with out_bf16) [B*T][ldo]
//   rows_bf16 (16-bit modes, T' <= 128): qkv bf16 [B*T][ldq], out bf16; one work-group per (utterance, head)
//   streaming (chunk by chunk): T query frames per utterance (row_len: the valid ones), K / V history hist [B][cap][2 D] appended
//   to in place, device-side chunk counter `step`
struct AttArgs {
  const void* qkv = nullptr; int ldq = 0; const float* pmat = nullptr; int ldp = 0; const float *pos_u = nullptr, *pos_v = nullptr;
  const int32_t* row_len = nullptr; int B = 0, T = 0, H = 0, dk = 0; float scale = 1.f; void* out = nullptr; int ldo = 0, out_bf16 = 0;
  const int32_t* row0 = nullptr; int chunk = 0, left_chunks = 0;   // chunk > 0: static chunk mask (utils/mask.py:42-75)
  int rows_bf16 = 0;
  int streaming = 0; float* hist = nullptr; int cap = 0; const int32_t* step = nullptr;
  int slot_max_chunks = -1;   // >= 0: slot mode, step [B] = one counter per slot, max_frames / T
};
int launch_relpos_attention(const AttArgs& a, hipStream_t stream);
bool relpos_attention_dual_fusable(const AttArgs& a, const AttArgs& b);
int launch_relpos_attention_dual(const AttArgs& a, const AttArgs& b, hipStream_t stream);
bool relpos_attention_bf16_supports(int T, int dk);
int init_relpos_attention_bf16_kernels();

// ---- conv module / subsampling (conv.hip) ----
int launch_pad2d(const float* x, size_t outer, int H, int W, int pre_h, int post_h, int pre_w, int post_w, float* y, hipStream_t stream);
int launch_advance_counter(int32_t* counter, int by, hipStream_t stream);
int launch_fill_rows(const float* row, int D, float* out, size_t rows, hipStream_t stream);
// streaming in slot mode (rowops.hip): per-slot words pos / status / frames [B] each
int launch_advance_slots(int32_t* pos, int32_t* status, int32_t* frames, const int32_t* chunk_len, int B, int C, int max_chunks,
                         hipStream_t stream);
constexpr int kMaxStreamBlocks = 64;      // conformer blocks (embed + main) one restart launch covers
struct SlotResetArgs {
  int32_t *pos = nullptr, *status = nullptr, *frames = nullptr;
  const int32_t* slots = nullptr; int n = 0;      // device list of the slots to restart (values outside [0, B) are skipped)
  int B = 0, K = 0, D = 0, n_blocks = 0;
  float* conv[kMaxStreamBlocks];                  // per block the ping-pong conv cache [2][B][K-1][D]
  const float* fill[kMaxStreamBlocks];            // per block its left_fill row [D]
};
int launch_reset_slots(const SlotResetArgs& a, hipStream_t stream);
int launch_slot_positions(const int32_t* status, const int32_t* frames, int B, int32_t* out, hipStream_t stream);
// The conv module's depthwise conv + LayerNorm + SiLU: one record per problem (what the engine keeps per stage and the C ABI fills
// from its descriptor), one check, one launcher; two problems of one instantiation can share a launch
struct DwArgs {
  const float *z = nullptr, *w_kc = nullptr, *bias = nullptr, *gamma = nullptr, *beta = nullptr; float eps = 1e-5f;
  int B = 0, T = 0, D = 0, K = 0; float* out = nullptr; int out_bf16 = 0;
  const int32_t *pad_of = nullptr, *row0 = nullptr, *row_len = nullptr;
  const float* causal_left_fill = nullptr;   // non-null: causal conv (lorder K-1), the row [D] every frame left of frame 0 holds
  int glu_ldz = 0;   // > 0: z is pointwise_conv1's raw [B*T][glu_ldz] output (value | gate columns), GLU applied as the taps are loaded
  int glu_sig = 0;   // (with glu_ldz) the gate columns hold sigmoid(gate) already (GemmParams::sig_col0): every tap is one multiply
  // chunk-by-chunk (streaming) form of the causal conv: cache_pair [2][B][K-1][D], chunk counter and valid frames on the device
  int streaming = 0; float* cache_pair = nullptr; const int32_t *step = nullptr, *chunk_len = nullptr;
  int slot_max_chunks = -1;   // >= 0: slot mode, step [B]
};
int launch_dwconv_ln_silu(const DwArgs& a, hipStream_t stream);
bool dwconv_glu_in_supports(int D, int K, bool causal_or_stream, int out_bf16, int ldz);   // what the GLU-on-load form takes
bool dwconv_dual_fusable(const DwArgs& a, const DwArgs& b);
int launch_dwconv_ln_silu_dual(const DwArgs& a, const DwArgs& b, hipStream_t stream);
// packed (padding-free) rows of a ragged batch (rowops.hip): plan from the valid lengths; padded output from packed rows
int launch_pack_plan(int32_t* len, int B, int T, int32_t* row0, int32_t* pad_of, hipStream_t stream,
                     const int32_t* feat_len = nullptr);   // feat_len: form the subsampled lengths here too (len becomes an output)
int launch_unpack_rows(const float* in, const int32_t* row0, int B, int T, int n, float* out, hipStream_t stream);
// The subsamplers' first conv: one record per problem (what the engine keeps per stage and the C ABI fills from its descriptor),
// one check, one launcher; two problems on the same input shape can share a launch
struct Conv1Args {
  const float *feat = nullptr, *w9c = nullptr, *bias = nullptr, *cmvn_mean = nullptr, *cmvn_istd = nullptr;
  int B = 0, T = 0, idim = 0, C = 0; float* out = nullptr; int relu = 1, out_bf16 = 0;
  const int32_t* feat_len = nullptr; int32_t* lens_out = nullptr;   // feat_len: the launch also forms the subsampled lengths
  // input channels (1..3): a frame's idim columns are in_ch blocks of Fc = idim / in_ch bins, w9c is [in_ch * 9][C] with row
  // ch * 9 + kh * 3 + kw, the output has F1 = (Fc - 3) / 2 + 1 columns
  int in_ch = 1;
};
int launch_conv1_relu(const Conv1Args& a, hipStream_t stream);
bool conv1_dual_fusable(const Conv1Args& a, const Conv1Args& b);
int launch_conv1_relu_dual(const Conv1Args& a, const Conv1Args& b, hipStream_t stream);
int launch_cmvn(const float* x, const int32_t* len, const float* mean, const float* istd, int B, int T, int D,
                float* y, hipStream_t stream);
int launch_log_softmax_bias(const float* x, const float* bias, float* y, size_t rows, int n, hipStream_t stream);
// decode.hip: CTC search on the logits + the streaming operators
int launch_ctc_greedy(const float* logits, const int32_t* len, int B, int T, int V, int blank, int32_t* frame_ids,
                      int32_t* tokens, int32_t* n_tokens, hipStream_t stream);
int launch_ctc_topk(const float* logits, size_t rows, int V, int k, float* top_logp, int32_t* top_idx, hipStream_t stream);
int ctc_prefix_beam_search_host(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, int32_t* n_hyps);
int launch_ctc_argmax(const float* logits, size_t rows, int V, int32_t* ids, hipStream_t stream);
// ctc_beam.hip: batched resumable prefix beam search and the streaming greedy search on the device
// The prefix beam search has three forms: m3_ctc_beam_*, m3_ctc_beam_ctx_* (context biasing) and m3_ctc_beam_lm_*
// (biasing and an n-gram LM).  BeamCall names everything any of their entry points receives; what a call does not have stays zero.
enum class BeamForm { Plain, Ctx, Lm };
struct BeamCall {
  const char* who;               // the entry point's name in messages
  BeamForm form;
  const m3_ctc_beam_desc* d;
  void* state;                   // (nbest only reads it)
  size_t bytes;
  const int32_t* slots;          // reset: a device list of n utterances; nullptr = every utterance
  int n;
  const void* image;             // the context image, and each utterance's graph in it
  size_t image_bytes;
  const int32_t* graph_of;
  const void* lm_image;          // the LM image (or set), each utterance's switch (or member), the weights of the key
  size_t lm_bytes;
  const int32_t* lm_on;
  double alpha, beta;
  int use_eos;
  const float* top_logp;         // advance: [B][T_chunk][k] of m3_ctc_topk, and each row's real frames
  const int32_t* top_idx;
  int T_chunk;
  const int32_t* n_frames;
  int32_t *hyp_tokens, *hyp_len; // nbest
  float *hyp_score, *hyp_bonus, *hyp_lm;
  int32_t* n_hyps;
  hipStream_t stream;
};
size_t beam_state_need(const m3_ctc_beam_desc* d, BeamForm form);   // 0 (and the error set) on a bad descriptor
int beam_reset(const BeamCall& c);
int beam_advance(const BeamCall& c);
int beam_nbest(const BeamCall& c);
// ctc_align.hip: CTC forced alignment: emissions of the asked-for tokens, then trellis + backtrace + spans
size_t ctc_align_workspace_size(const m3_ctc_align_desc* d);
int launch_ctc_align_emit(const m3_ctc_align_desc* d, const float* logits, int ldl, const int32_t* row0, const int32_t* n_frames,
                          const int32_t* tokens, const int32_t* tok0, float* emit, hipStream_t stream);
int launch_ctc_align_path(const m3_ctc_align_desc* d, const float* emit, const int32_t* n_frames, const int32_t* tokens,
                          const int32_t* tok0, void* workspace, size_t ws_bytes, float* score, int32_t* status, int32_t* state,
                          int32_t* tok_start, int32_t* tok_end, int32_t* tok_peak, float* tok_logp, hipStream_t stream);
// Context biasing of the prefix beam search (include/m3asr.h, "context set"): one image of 4-byte words,
//   [magic, G, V, words] then G x [n_states, A, cls, next, delta, pot (word offsets of the tables), 0, 0] then the tables.
constexpr int32_t kCtxMagic = 0x5843334d;   // "M3CX"
constexpr int kCtxMaxGraphs = 1024, kCtxMaxStates = 65536;
constexpr size_t kCtxMaxBytes = (size_t)64 << 20;
enum { CTX_MAGIC = 0, CTX_G = 1, CTX_V = 2, CTX_WORDS = 3, CTX_HDR_WORDS = 4 };
enum { CTXG_STATES = 0, CTXG_A = 1, CTXG_CLS = 2, CTXG_NEXT = 3, CTXG_DELTA = 4, CTXG_POT = 5, CTXG_WORDS = 8 };
struct CtxGraph {
  const int32_t* cls;    // [V]
  const int32_t* next;   // [n_states][A]
  const float* delta;    // [n_states][A]
  const float* pot;      // [n_states]
  int n_states, A, V;
};
// Graph g of an image of `words` words, for the host and the device alike.  False unless the header, g and all four tables
// lie inside the image and the limits hold: no address is formed from a value that failed its check.  (Table ENTRIES are
// checked by ctc_context_validate on the host, and once more where the device search uses one as an index.)
__host__ __device__ inline bool ctx_graph_view(const int32_t* image, long long words, int g, CtxGraph* out) {
  if (image == nullptr || words < CTX_HDR_WORDS || image[CTX_MAGIC] != kCtxMagic) return false;
  const long long G = image[CTX_G], V = image[CTX_V];
  if (G < 0 || G > kCtxMaxGraphs || V < 1 || CTX_HDR_WORDS + G * CTXG_WORDS > words || g < 0 || g >= G) return false;
  const int32_t* h = image + CTX_HDR_WORDS + (long long)g * CTXG_WORDS;
  const long long ns = h[CTXG_STATES], A = h[CTXG_A], first = CTX_HDR_WORDS + G * CTXG_WORDS;
  if (ns < 1 || ns > kCtxMaxStates || A < 1 || A > V + 1 || A > kCtxMaxStates) return false;
  const long long off[4] = {h[CTXG_CLS], h[CTXG_NEXT], h[CTXG_DELTA], h[CTXG_POT]};
  const long long len[4] = {V, ns * A, ns * A, ns};
  for (int i = 0; i < 4; ++i)
    if (off[i] < first || off[i] > words || len[i] > words - off[i]) return false;
  out->cls = image + off[0];
  out->next = image + off[1];
  out->delta = (const float*)(image + off[2]);
  out->pot = (const float*)(image + off[3]);
  out->n_states = (int)ns;
  out->A = (int)A;
  out->V = (int)V;
  return true;
}
int ctc_context_validate(const void* image, size_t bytes, int V);   // decode.hip, host only
int ctc_prefix_beam_search_ctx_host(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                    const void* image, size_t image_bytes, int graph, int32_t* hyp_tokens, int32_t* hyp_len,
                                    float* hyp_score, float* hyp_bonus, int32_t* hyp_state, int32_t* n_hyps);
// n-gram LM shallow fusion of the prefix beam search (include/m3asr.h, "LM image"): one image of 4-byte words,
//   [magic, version, V, order, n_states, n_arcs, start, unk_logp bits, the tables' word offsets (LMT_* order), words, 0, 0]
// then the tables of a deterministic back-off automaton over context states (m3asr/lm.py compiles ARPA files into it).
constexpr int32_t kLmMagic = 0x4d4c334d;   // "M3LM"
constexpr int32_t kLmVersion = 1;
constexpr int kLmMaxOrder = 8, kLmMaxStates = 1 << 26;
constexpr size_t kLmMaxBytes = (size_t)1 << 30;
enum { LM_MAGIC = 0, LM_VERSION = 1, LM_V = 2, LM_ORDER = 3, LM_STATES = 4, LM_ARCS = 5, LM_START = 6, LM_UNK = 7, LM_TABLES = 8,
       LM_WORDS = 17, LM_HDR_WORDS = 20 };
enum { LMT_UNI_LOGP = 0, LMT_UNI_NEXT, LMT_ARC_BEGIN, LMT_ARC_TOK, LMT_ARC_NEXT, LMT_ARC_LOGP, LMT_BO_STATE, LMT_BO_WEIGHT,
       LMT_FINAL, LMT_COUNT };
struct LmView {
  const float* uni_logp;      // [V]             state 0's arcs are dense
  const int32_t* uni_next;    // [V]
  const int32_t* arc_begin;   // [n_states + 1]  arcs of state s: [arc_begin[s], arc_begin[s + 1])
  const int32_t* arc_tok;     // [n_arcs]        strictly ascending inside a state
  const int32_t* arc_next;    // [n_arcs]
  const float* arc_logp;      // [n_arcs]
  const int32_t* bo_state;    // [n_states]      bo_state[s] < s for s >= 1
  const float* bo_weight;     // [n_states]
  const float* fin;           // [n_states]      log P(</s> | state), back-off resolved
  int V, order, n_states, n_arcs, start;
  float unk_logp;
};
// The tables of an image of `words` words, for the host and the device alike.  False unless the header and all nine tables
// lie inside the image and the limits hold: no address is formed from a value that failed its check.  (Table ENTRIES are
// checked by ctc_lm_validate on the host, and once more where a search uses one as an index.)
__host__ __device__ inline bool lm_view(const int32_t* image, long long words, LmView* out) {
  if (image == nullptr || words < LM_HDR_WORDS || image[LM_MAGIC] != kLmMagic || image[LM_VERSION] != kLmVersion) return false;
  const long long V = image[LM_V], order = image[LM_ORDER], ns = image[LM_STATES], na = image[LM_ARCS], start = image[LM_START];
  if (V < 1 || order < 1 || order > kLmMaxOrder || ns < 1 || ns > kLmMaxStates || na < 0 || start < 0 || start >= ns) return false;
  const long long len[LMT_COUNT] = {V, V, ns + 1, na, na, na, ns, ns, ns};
  for (int i = 0; i < LMT_COUNT; ++i) {
    const long long off = image[LM_TABLES + i];
    if (off < LM_HDR_WORDS || off > words || len[i] > words - off) return false;
  }
  out->uni_logp = (const float*)(image + image[LM_TABLES + LMT_UNI_LOGP]);
  out->uni_next = image + image[LM_TABLES + LMT_UNI_NEXT];
  out->arc_begin = image + image[LM_TABLES + LMT_ARC_BEGIN];
  out->arc_tok = image + image[LM_TABLES + LMT_ARC_TOK];
  out->arc_next = image + image[LM_TABLES + LMT_ARC_NEXT];
  out->arc_logp = (const float*)(image + image[LM_TABLES + LMT_ARC_LOGP]);
  out->bo_state = image + image[LM_TABLES + LMT_BO_STATE];
  out->bo_weight = (const float*)(image + image[LM_TABLES + LMT_BO_WEIGHT]);
  out->fin = (const float*)(image + image[LM_TABLES + LMT_FINAL]);
  out->V = (int)V;
  out->order = (int)order;
  out->n_states = (int)ns;
  out->n_arcs = (int)na;
  out->start = (int)start;
  out->unk_logp = ((const float*)image)[LM_UNK];
  return true;
}
// An LM SET (include/m3asr.h, "LM set"): G complete LM images behind one header and a directory, one device image.
//   [magic, version, V, G, total words, 0, 0, 0]   G x [offset words, n words, scale (float bits), 0]   the member images
constexpr int32_t kLmSetMagic = 0x534c334d;   // "M3LS"
constexpr int32_t kLmSetVersion = 1;
constexpr int kLmSetMaxMembers = 64;
constexpr size_t kLmSetMaxBytes = (size_t)1 << 31;
enum { LMS_MAGIC = 0, LMS_VERSION = 1, LMS_V = 2, LMS_G = 3, LMS_WORDS = 4, LMS_HDR_WORDS = 8 };
enum { LMS_E_OFFSET = 0, LMS_E_WORDS = 1, LMS_E_SCALE = 2, LMS_ENTRY_WORDS = 4 };
__host__ __device__ inline bool lm_is_set(const int32_t* image, long long words) {
  return image != nullptr && words >= LMS_HDR_WORDS && image[LMS_MAGIC] == kLmSetMagic;
}
// Member j of a set of `words` words as (first word, word count, scale).  False unless the set's header, the directory entry
// and the member's extent pass their range checks: no address is formed from a value that failed one.  (What lies INSIDE the
// member is lm_view's to check.)
__host__ __device__ inline bool lm_set_entry(const int32_t* image, long long words, long long j, const int32_t** member,
                                             long long* member_words, float* scale) {
  if (!lm_is_set(image, words) || image[LMS_VERSION] != kLmSetVersion) return false;
  const long long V = image[LMS_V], G = image[LMS_G], total = image[LMS_WORDS];
  if (V < 1 || G < 1 || G > kLmSetMaxMembers || total > words || total < LMS_HDR_WORDS + G * LMS_ENTRY_WORDS) return false;
  if (j < 0 || j >= G) return false;
  const int32_t* e = image + LMS_HDR_WORDS + j * LMS_ENTRY_WORDS;
  const long long off = e[LMS_E_OFFSET], n = e[LMS_E_WORDS];
  const float s = ((const float*)e)[LMS_E_SCALE];
  if (off < LMS_HDR_WORDS + G * LMS_ENTRY_WORDS || (off & 3) != 0 || n < LM_HDR_WORDS || off > total || n > total - off) return false;
  if (!(s > 0.f) || !(s <= 3.4028234663852886e38f)) return false;          // finite and positive; NaN fails both
  *member = image + off;
  *member_words = n;
  *scale = s;
  return true;
}
// The tables an utterance with the switch `on` walks, resolved ONCE per utterance (all loads are uniform): false = it runs
// without the LM.  A single image: on != 0 and lm_view, as ever.  A set: on = j in [1, G] picks member j - 1, whose view must
// also be over the set's V; *alpha then becomes *alpha * (double)scale, one double product.  Any other value: off.
// (base, words, scale) are picked FIRST and lm_view runs once, on the chosen base: one copy of the header checks in the
// kernel, and from there on the walk cannot tell a member from a single image.  A single image above the single image's
// size limit is off, as the launch checks had it before they had to admit a set's size.
#ifndef M3_LM_SET_PICK_ATTR
#define M3_LM_SET_PICK_ATTR inline
#endif
#ifndef M3_LM_SET_EXPECT
#define M3_LM_SET_EXPECT 0
#endif
__host__ __device__ M3_LM_SET_PICK_ATTR bool lm_select(const int32_t* image, long long words, int on, LmView* out, double* alpha) {
  if (on == 0) return false;
  const int32_t* base = image;
  long long n = words, want_V = 0;
  if (__builtin_expect(lm_is_set(image, words), M3_LM_SET_EXPECT)) {
    float scale;
    if (!lm_set_entry(image, words, (long long)on - 1, &base, &n, &scale)) return false;
    want_V = image[LMS_V];
    *alpha = *alpha * (double)scale;
  } else if (words > (long long)(kLmMaxBytes / 4)) {
    return false;
  }
  return lm_view(base, n, out) && (want_V == 0 || out->V == want_V);
}
__host__ __device__ inline int lm_in_range(int v, int n) { return (unsigned)v < (unsigned)n ? v : 0; }
// position of tok among the arcs [lo, hi) (0 <= lo <= hi <= n_arcs, checked by the caller), or -1
__host__ __device__ inline int lm_find(const LmView& m, int lo, int hi, int tok) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1, t = m.arc_tok[mid];
    if (t == tok) return mid;
    if (t < tok) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}
// The arcs of state st as a checked range: an arc_begin pair that is not 0 <= lo <= hi <= n_arcs means "no arcs".
__host__ __device__ inline void lm_arcs(const LmView& m, int st, int* lo, int* hi) {
  *lo = m.arc_begin[st];
  *hi = m.arc_begin[st + 1];
  if (*lo < 0 || *hi > m.n_arcs || *lo > *hi) *lo = *hi = 0;
}
// The last level of every walk: state 0, whose arcs are dense.  A token outside [0, V) is one the LM does not know.
__host__ __device__ inline double lm_step_root(const LmView& m, double w, int tok, int* next) {
  if ((unsigned)tok < (unsigned)m.V) {
    *next = lm_in_range(m.uni_next[tok], m.n_states);
    return w + (double)m.uni_logp[tok];
  }
  *next = 0;
  return w + (double)m.unk_logp;
}
// THE SCORE CONTRACT: log P(tok | state) and the state reached.  From `state` down its back-off chain (bo_state[s] < s, so
// the walk ends; a validated image has at most order - 1 levels above state 0), the back-off weights summed in double in
// walk order, then the arc's value added.  *backoffs (optional): levels left without a match.
__host__ __device__ inline double lm_step(const LmView& m, int state, int tok, int* next, int* backoffs = nullptr) {
  double w = 0.0;
  int st = state, lvl = 0;
  for (; st != 0 && lvl < kLmMaxOrder; ++lvl) {
    int lo, hi;
    lm_arcs(m, st, &lo, &hi);
    const int i = lm_find(m, lo, hi, tok);
    if (i >= 0) {
      if (backoffs) *backoffs = lvl;
      *next = lm_in_range(m.arc_next[i], m.n_states);
      return w + (double)m.arc_logp[i];
    }
    w += (double)m.bo_weight[st];
    const int nb = m.bo_state[st];
    st = nb >= 0 && nb < st ? nb : 0;
  }
  if (backoffs) *backoffs = lvl;
  return lm_step_root(m, w, tok, next);
}
int ctc_lm_validate(const void* image, size_t bytes, int V);   // decode.hip, host only; a single image or a set
int ctc_lm_set_member(const void* image, size_t bytes, int j, const void** member, size_t* member_bytes, float* scale);   // host only
int ctc_prefix_beam_search_lm_host(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                   const void* image, size_t image_bytes, int graph, const void* lm_image, size_t lm_bytes,
                                   double alpha, double beta, int use_eos, int32_t* hyp_tokens, int32_t* hyp_len,
                                   float* hyp_score, float* hyp_bonus, int32_t* hyp_state, float* hyp_lm, int32_t* n_hyps);
size_t ctc_greedy_stream_state_size(const m3_ctc_greedy_desc* d);
int launch_ctc_greedy_stream_reset(const m3_ctc_greedy_desc* d, void* state, size_t bytes, hipStream_t stream,
                                   const int32_t* slots = nullptr, int n = 0);
int launch_ctc_greedy_stream_advance(const m3_ctc_greedy_desc* d, void* state, size_t bytes, const float* logits, int T_chunk,
                                     int V, const int32_t* n_frames, int32_t* frame_ids, hipStream_t stream);
int launch_ctc_greedy_stream_tokens(const m3_ctc_greedy_desc* d, const void* state, size_t bytes, int32_t* tokens,
                                    int32_t* n_tokens, hipStream_t stream);
// ctc_wfst.hip: token-passing beam search over a compiled graph
int wfst_validate(const void* image, size_t bytes, int V);   // host only
size_t wfst_search_state_size(const m3_wfst_search_desc* d);
int launch_wfst_search_reset(const m3_wfst_search_desc* d, void* state, size_t bytes, const void* image, size_t image_bytes,
                             const int32_t* slots, int n, hipStream_t stream);
int launch_wfst_search_advance(const m3_wfst_search_desc* d, void* state, size_t bytes, const void* image, size_t image_bytes,
                               const float* logp, int ld, int T_chunk, const int32_t* n_frames, hipStream_t stream);
int launch_wfst_search_result(const m3_wfst_search_desc* d, const void* state, size_t bytes, const void* image, size_t image_bytes,
                              int final, int max_words, int32_t* words, int32_t* frames, int32_t* n_words, float* cost,
                              int32_t* flags, int32_t* status, hipStream_t stream);
// ctc_wfst_skip.hip: CTC blank-frame skipping in front of that search
size_t wfst_skip_state_size(const m3_wfst_skip_desc* d);
int launch_wfst_skip_reset(const m3_wfst_skip_desc* d, void* state, size_t bytes, const int32_t* slots, int n, hipStream_t stream);
int launch_wfst_skip_select(const m3_wfst_skip_desc* d, void* state, size_t bytes, const float* logp, int ld, int T_chunk,
                            const int32_t* n_frames, float* out, int ld_out, int32_t* n_kept, hipStream_t stream);
int launch_wfst_skip_map_frames(const m3_wfst_skip_desc* d, const void* state, size_t bytes, int32_t* frames, int ld_frames,
                                const int32_t* n_words, hipStream_t stream);
int launch_wfst_skip_counts(const m3_wfst_skip_desc* d, const void* state, size_t bytes, int32_t* seen, int32_t* kept,
                            hipStream_t stream);
// endpoint detection next to the two searches (ctc_beam.hip)
size_t ctc_endpoint_state_size(const m3_ctc_endpoint_desc* d);
int launch_ctc_endpoint_reset(const m3_ctc_endpoint_desc* d, void* state, size_t bytes, hipStream_t stream,
                              const int32_t* slots = nullptr, int n = 0);
int launch_ctc_endpoint_advance(const m3_ctc_endpoint_desc* d, void* state, size_t bytes, const float* top_logp,
                                const int32_t* top_idx, int T_chunk, int k, const int32_t* n_frames, hipStream_t stream);
int launch_ctc_endpoint_read(const m3_ctc_endpoint_desc* d, const void* state, size_t bytes, int32_t* info, hipStream_t stream);
int launch_cat_split_cache(const void* in_cache, const void* input, int B, int cache_dim, int input_dim, void* output,
                           void* out_cache, hipStream_t stream);
int launch_att_stream_softmax(const float* scores, const int32_t* decode_frame_num, const int32_t* mask_idx, int B, int N,
                              int ld, int cache_len, float scale, float* out, hipStream_t stream);
int launch_rel_positional_encoding(const float* x, const float* pe, int pe_len, const int32_t* frame_num, int max_offset,
                                   float scale, int B, int T, int D, float* y, float* pos_emb, int32_t* frame_num_out,
                                   hipStream_t stream);
int launch_depthwise_conv1d_nct(const float* x, const float* w, const float* bias, int B, int C, int T, int K,
                                int pad, float* y, hipStream_t stream);

// fbank.hip: Kaldi-style log-Mel filter bank, samples -> feature frames
size_t fbank_tables_bytes();
int fbank_tables_build(int num_mel_bins, double sample_rate, double low_freq, double high_freq, void* host_image);
int launch_fbank(const void* tables, const void* pcm, int pcm_is_int16, int ld_pcm, const int32_t* n_samples, int B, int T,
                 int num_mel_bins, float* feat, int ld_feat, int32_t* feat_len, hipStream_t stream);

// resample.hip: Kaldi LinearResample, samples at any rate -> samples at the feature rate
size_t resample_tables_bytes(int rate_in, int rate_out);                  // 0 (and the error string) when the pair is refused
int resample_tables_build(int rate_in, int rate_out, void* host_image);
long resample_num_samples(int rate_in, int rate_out, long n_in, int flush);
void resample_input_span(int rate_in, int rate_out, long out0, long n_out, long* first_in, long* end_in);
int launch_resample(const void* tables, const void* pcm, int pcm_is_int16, int channels, int channel, int ld_pcm,
                    const int64_t* in0, const int32_t* n_in, const int64_t* out0, const int32_t* n_out, int B, int N_out,
                    float* out, int ld_out, hipStream_t stream);

// deltas.hip: Kaldi DeltaFeatures (add-deltas), static frames -> static | delta | delta-delta
constexpr int DELTAS_MAX_CONTEXT = 8;                                     // order * window at most
int deltas_options_ok(int order, int window);
int deltas_tables_build(int order, int window, float* scales);           // (order + 1) rows of 2 * DELTAS_MAX_CONTEXT + 1 floats
int launch_add_deltas(const float* feat, long ld_feat, long bs_feat, int T_in, const int32_t* n_in, const int32_t* lead,
                      const int32_t* n_out, int B, int T_out, int bins, int order, int window, float* out, long ld_out,
                      long bs_out, int32_t* out_len, hipStream_t stream);

// vad.hip: Kaldi compute-vad on frame log-energy, a segmenter on its flags, and the cut of feature rows into an engine batch
// 
constexpr int VAD_MAX_CONTEXT = 32;
int vad_options_ok(float energy_mean_scale, int context, float proportion_threshold);
int segment_options_ok(int min_silence, int min_speech, int pad, int max_segment, int split_search);
int launch_vad_log_energy(const void* pcm, int pcm_is_int16, long ld_pcm, const int32_t* n_samples, int B, int T, float* log_energy,
                          long ld_out, int32_t* len_out, hipStream_t stream);
int launch_vad_decide(const float* log_energy, long ld_e, const int32_t* lens, int B, int T, float energy_threshold,
                      float energy_mean_scale, int context, float proportion_threshold, uint8_t* flags, long ld_flags,
                      float* threshold_out, hipStream_t stream);
int launch_vad_segments(const uint8_t* flags, long ld_flags, const float* log_energy, long ld_e, const int32_t* lens, int B, int T,
                        int min_silence, int min_speech, int pad, int max_segment, int split_search, int32_t* segments,
                        int capacity, int32_t* n_segments, hipStream_t stream);
int launch_segment_gather(const float* src, long ld_src, int T_all, const int32_t* jobs, int B, int T_max, int cols, float* dst,
                          long ld_dst, long bs_dst, int32_t* len_out, hipStream_t stream);

}  // namespace m3
