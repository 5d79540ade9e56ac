// Skinny fp32 GEMM  Y[M,N] = epilogue( prologue(A)[M,K] . W[N,K]^T )  on v_mfma_f32_16x16x4_f32.
//
// Replaces the TensorRT-native layers of the reference hot path (no reference kernel source):
//   Linear  = constant-weight matmul + bias add   (TRTAPI++/python/trt_helper/torch_network_helper.py:573-605)
//   Conv1d point-wise (k=1)                        (torch_network_helper.py:199-225)
//   Conv2d 3x3 stride 2 (second subsampling conv)  (torch_network_helper.py:227-251) as implicit GEMM
//   router matmul on cat([embed, x])               (trainer_3m_fix/layer/positionwise_feed_forward.py:169-180,225)
// with the surrounding element-wise layers fused as prologue / epilogue:
//   LayerNorm on the A rows (layer_norm_kernel.cu:33-139, but WITH eps),
//   masked_fill(0) of padded frames before / after (masked_fill_kernel.cu:27-54),
//   bias, ReLU / SiLU / GLU (glu_kernel.cu:26-44), uniform scale + residual add
//   (tensor_network_helper.py:406-471).
//
// Shape regime: M = B*T' tokens (50 .. ~2000), N, K in 512..4608: every weight element is used by
// only M rows, so this is a weight-streaming kernel whose run time at M = 50 is a few microseconds,
// i.e. it is bound by memory latency and by the number of instructions a wave issues.  Layout:
// one workgroup = 16 output columns (x2 for GLU) x 16*MT rows; its NW waves split K round-robin in
// 16-deep steps; each wave streams its W rows and A rows straight into VGPRs (float4 per lane = 16
// rows x 64 B per instruction), two groups of G steps in flight, all loads unconditional (clamped
// addresses: a branch around a load makes hipcc wait per load); partial tiles are summed through LDS in
// a fixed order (no atomics -> bitwise reproducible).  Small M is split into 16-row tiles so a
// 50-token utterance spreads over 128-256 workgroups; the tiles of one weight column block sit on
// the same XCD (blockIdx % 8) so the weight tile is fetched from HBM once.
//
// LayerNorm has two forms:
//  * LN_EPI (engine): the affine is folded into W / bias when the plan is packed, and the
//    normalisation moves to the OUTPUT side:  y_n = rstd_m * (acc_mn - mean_m * wsum_n) + bias'_n  with
//    wsum_n = sum_k W'_nk.  The GEMM runs on the raw rows, the row sums (sum a, sum a^2) are taken from
//    the A fragments already in registers, so LayerNorm costs no extra memory round trip and no barrier.
//  * LN_PRO (generic m3_linear with gamma / beta): statistics (two-pass) + affine applied to the A
//    fragments before the MFMAs; can also write the normalised rows out (ln_out).
#include "common.h"
#include "gemm_epilogue.h"
#include "kernels.h"

// -DM3_GEMM_DIAG: phase stamps (s_memtime) of every work-group of gemm_f32_kernel into a debug buffer (tools/diag_gemm_f32.py)
#ifdef M3_GEMM_DIAG
#define M3_GDIAG(...) __VA_ARGS__
#else
#define M3_GDIAG(...)
#endif

namespace m3 {

M3_GDIAG(__device__ unsigned long long g_gemm_dbg[2048 * 8];)

enum { LN_NONE = GEMM_LN_NONE, LN_EPI = GEMM_LN_EPI, LN_PRO = GEMM_LN_PRO };

// NW = waves per workgroup = K-split factor (4 / 8 / 16 for K ~ 512 / 1024 / >= 2048).
// NBUF = 1 when a wave's share of K fits one load group (K <= 16*NW*G: every block GEMM of the model): half the
// staging registers -> <= 128 VGPRs -> 4 waves per SIMD, so kernels of other streams can share the CU.
// The kernel body as a device function of (parameter block, work-group id): gemm_f32_kernel runs one problem,
// gemm_f32_dual_kernel two INDEPENDENT problems of the same instantiation in one launch (work-groups [0, n0) the first,
// the rest the second) -- the embed encoder and the main encoder's first block do not depend on each other until that block's
// router, so their GEMMs can share launches (engine.hip: "horizontal fusion"; a launch saved is ~6 us of a B = 1 forward).
// ACCI (GemmParams::acc_init; the router on cat([embed, LN(x)])): the wave's A-half K-steps -- the first half of its one load
// group, K1 == K / 2 == 8 * NW * G by the plan's check -- were run by router_embed_prefix_kernel, which left (acc, acc2) as they
// stand after them.  The wave loads the pair with its operand group and starts at step G / 2: the skipped steps are not in the
// instantiation at all.  wave w walks steps w, w + NW, ... in increasing order, so an MFMA chain cut there yields the same bits.
// WF (GemmParams::w_frag; the plan: plain A, N (GLU: N / 2) and K multiples of 16): W in MFMA-fragment order.  Only the weight
// addresses of load_group differ; a template argument, so that the row-major instantiations are the code they were.
template <int MT, bool GLU, int NW, bool CONV, int LN, int NBUF, bool ACCI = false, bool WF = false>
__device__ __forceinline__ void gemm_f32_body(const GemmParams& p, const int bid) {
  static_assert(!WF || (!CONV && !ACCI), "fragment-ordered W: plain A only");
  constexpr int NT = GLU ? 2 : 1;
  constexpr int G = gemm_group_steps(MT, NT, NW);
  constexpr int I0 = ACCI ? G / 2 : 0;   // first K-step of the load group this instantiation runs
  static_assert(!ACCI || (MT == 1 && !GLU && !CONV && NBUF == 1 && G % 2 == 0), "acc_init: the one-group 16-row concat form only");
  constexpr int RW = (16 * MT) / NW;   // rows per wave in the LN_PRO prologue (>= 1)
  static_assert(RW >= 1, "more waves than rows");
  __shared__ float red[NW][MT * NT][256];
  __shared__ float stats[16 * MT][2];
  __shared__ float rsum[LN == LN_EPI ? NW : 1][16 * MT][2];
  __shared__ __attribute__((aligned(16))) float ln_g[LN == LN_PRO ? 1024 : 4], ln_b[LN == LN_PRO ? 1024 : 4];

  M3_GDIAG(unsigned long long dg[8]; dg[0] = __builtin_amdgcn_s_memtime();)
  // ONE batch of kernel-argument loads.  hipcc fetches each field of the by-value parameter block where it is first used: the
  // prologue was ~8 dependent rounds of s_load + s_waitcnt (2 400 cycles = 1.1 us before the first global load was issued,
  // in-kernel stamps, tools/diag_gemm_f32.py).  Naming the fields as scalar operands of one empty asm statement makes it load
  // them together, one wait.  ONE statement: with the fields an instantiation adds in statements of their own the loads came out
  // as two batches with a wait between them.  A statement takes 30 operands, so the 32-bit fields go in pairs;
  // a field the instantiation never reads is a constant 0 here and is not loaded.
  {
    auto pk = [](int lo, int hi) { return (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32); };
    constexpr bool EPI = LN == LN_EPI, PRO = LN == LN_PRO;
    asm volatile("" ::"s"(p.A), "s"(p.W), "s"(p.bias), "s"(p.Y), "s"(p.m_dev), "s"(p.resid), "s"(p.row_len),
                 "s"(pk(p.lda, p.ldy)), "s"(pk(p.M, p.N)), "s"(pk(p.K, p.mode)), "s"(pk(p.n_tiles, p.m_tiles)),
                 "s"(pk(p.xcd_swizzle, p.ldr)), "s"(pk(p.act, __float_as_int(p.alpha))), "s"(pk(p.mask_in, p.mask_out)),
                 "s"(pk(p.rows_per_batch, p.sig_col0)), "s"(pk(p.one_run, LN != LN_NONE ? __float_as_int(p.ln_eps) : 0)),
                 "s"(pk((int)p.div_m_tiles.mul, p.div_m_tiles.shift)), "s"(pk((int)p.div_n_tiles.mul, p.div_n_tiles.shift)),
                 "s"(pk((int)p.div_rpb.mul, p.div_rpb.shift)),
                 "s"(ACCI ? p.acc_init : nullptr), "s"(EPI ? p.ln_wsum : PRO ? p.ln_gamma : nullptr),
                 "s"(EPI ? p.ln_wbeta : PRO ? p.ln_beta : nullptr), "s"(PRO ? p.ln_out : nullptr),
                 "s"(PRO ? pk(p.ld_ln_out, p.ln_on_a2) : 0ull), "s"(CONV ? nullptr : p.A2),
                 "s"(CONV ? pk(p.conv_T1, p.conv_F1) : pk(p.lda2, p.K1)), "s"(CONV ? pk(p.conv_T2, p.conv_F2) : 0ull),
                 "s"(CONV ? p.conv_C : 0));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int Nout = GLU ? (p.N >> 1) : p.N;

  // ---- workgroup -> (column tile, row tile); XCD-aware when the column-tile count allows ----
  // (the same order as `j % m_tiles, j / m_tiles` and `id % n_tiles, id / n_tiles`, on the scalar unit: the launcher's multiplier
  //  instead of a 30-instruction division sequence in front of the first address)
  int n_tile, m_tile;
  {
    const int id = bid;
    if (p.xcd_swizzle) {
      const int j = id >> 3;
      const int q = gemm_div_by(j, p.div_m_tiles);
      m_tile = j - q * p.m_tiles;
      n_tile = q * 8 + (id & 7);
    } else {
      m_tile = gemm_div_by(id, p.div_n_tiles);
      n_tile = id - m_tile * p.n_tiles;
    }
  }
  const int n0 = n_tile * 16;
  const int m0 = m_tile * (16 * MT);
  if (p.m_dev != nullptr && m0 > *p.m_dev) return;   // packed ragged batch: no live row in this tile
  const int ln_k0 = p.ln_on_a2 ? p.K1 : 0;             // first K index the LayerNorm applies to
  const int Kl = p.K - ln_k0;                          // LayerNorm row width

  // ---- per-lane row descriptors ----
  const float* arow[MT];
  const float* arow2[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = min(m0 + 16 * mt + col, p.M - 1);
    arow2[mt] = nullptr;
    if (CONV) {
      const int f2 = m % p.conv_F2;
      const int t2 = (m / p.conv_F2) % p.conv_T2;
      const int b = m / (p.conv_F2 * p.conv_T2);
      arow[mt] = p.A + ((size_t)(b * p.conv_T1 + 2 * t2) * p.conv_F1 + 2 * f2) * p.conv_C + 4 * kq;
    } else {
      arow[mt] = p.A + (size_t)m * p.lda + 4 * kq;
      if (p.mode == GEMM_A_CONCAT2) arow2[mt] = p.A2 + (size_t)m * p.lda2 + 4 * kq;
    }
  }
  // Row-major W: lane (col, kq) streams row n0 + col from column 4 * kq, 16 floats per K-step -- one wave instruction is 16 pieces
  // of 64 B from 16 rows.  Fragment order (WF): the lane streams its 16 bytes of the KB of (column tile, K-step), 256 floats per
  // K-step -- one instruction is one contiguous KB.  The same 16 bytes either way.
  const float* wrow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    wrow[t] = WF ? p.W + (size_t)(n_tile + t * (Nout >> 4)) * ((size_t)p.K << 4) + 4 * lane
                 : p.W + (size_t)min(n0 + t * Nout + col, p.N - 1) * p.K + 4 * kq;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr bool DUAL = MT * NT <= 2;
  f32x4 acc2[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc2[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float s1[MT], s2[MT];   // LN_EPI: this lane's share of sum(a), sum(a^2) of row (16*mt + col)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) s1[mt] = s2[mt] = 0.f;

  const int nsteps = p.K >> 4;
  auto a_offset = [&](int k) -> int {  // wave-uniform k (multiple of 16) -> element offset in the A row
    if (CONV) {
      const int seg = k / p.conv_C, c = k - seg * p.conv_C;
      const int kh = seg / 3, kw = seg - kh * 3;
      return (kh * p.conv_F1 + kw) * p.conv_C + c;
    }
    return k;
  };

  // two groups of G K-steps in flight (registers only; nothing is shared between waves)
  f32x4 wbuf[NBUF][G][NT], abuf[NBUF][G][MT];
  auto load_group = [&](int g, int buf) {
#pragma unroll
    for (int i = I0; i < G; ++i) {
      // steps past the end re-load the last step (results unused): no branch around the loads
      const int s = min(wave + NW * (G * g + i), nsteps - 1);
      const int k = s << 4;
#pragma unroll
      for (int t = 0; t < NT; ++t) wbuf[buf][i][t] = ldg4_w(wrow[t] + (WF ? (s << 8) : k));
      const bool second = ACCI || (!CONV && p.mode == GEMM_A_CONCAT2 && k >= p.K1);
      const int off = second ? (k - p.K1) : a_offset(k);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) abuf[buf][i][mt] = ldg4((second ? arow2[mt] : arow[mt]) + off);
    }
  };

  const int ngroups = (nsteps + NW * G - 1) / (NW * G);
  M3_GDIAG(dg[1] = __builtin_amdgcn_s_memtime();)
  // (Compile-time load offsets for the common exact shape -- one base address per row, no per-load address arithmetic -- were
  //  tried: issue-to-data time unchanged (4 830 vs 4 650 cycles): the loads are not bound by address arithmetic.  What they are
  //  bound by is WHICH bytes one instruction touches: row-major W gives 16 pieces of 64 B from 16 rows per wave instruction, and
  //  the group's issue-to-data span at M = 50, K = 512, cold W is 4 150-4 330 cycles; with W in fragment order (WF: one contiguous
  //  KB per instruction) it is 2 670-2 800 and the launch 4.40 us instead of 4.95.  The A loads keep the 16 x 64 B
  //  shape; the earlier reading "a CU keeps ~16 KB of misses in flight whatever the instruction stream" was wrong.)
  // ACCI: the LayerNorm statistics pass's row loads go out AHEAD of the operand group.  Loads return in issue order, and the
  // pass (two reductions, LDS, a barrier) stands between the last load and the first MFMA: behind the operand group it waited
  // for all of it.  Load order only; the arithmetic below is the same.
  f32x4 ln_v[16];
  auto load_stat_rows = [&](int c) {
    const int l16 = lane & 15;
    const int rloc = wave * RW + 4 * c + (lane >> 4);
    const int m = min(m0 + min(rloc, 16 * MT - 1), p.M - 1);
    const float* row = (p.ln_on_a2 ? p.A2 : p.A) + (size_t)m * (p.ln_on_a2 ? p.lda2 : p.lda);
#pragma unroll
    for (int j = 0; j < 8; ++j) ln_v[j] = ldg4(row + min(4 * (l16 + 16 * j), Kl - 4));
    if (Kl > 512) {   // (one wave-uniform branch: rows up to 512 wide have no element in the second eight fragments)
#pragma unroll
      for (int j = 8; j < 16; ++j) ln_v[j] = ldg4(row + min(4 * (l16 + 16 * j), Kl - 4));
    } else {
#pragma unroll
      for (int j = 8; j < 16; ++j) ln_v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  if (LN == LN_PRO && ACCI) load_stat_rows(0);
  load_group(0, 0);
  if (ACCI) {   // the accumulator pair as the A-half steps left it: requested with the operand group, needed at the first MFMA
    const float* pre = p.acc_init + ((size_t)((m_tile * p.n_tiles + n_tile) * NW + wave) * 2) * 256 + 4 * lane;
    acc[0][0] = ldg4(pre);
    acc2[0][0] = ldg4(pre + 256);
  }
  M3_GDIAG(dg[2] = __builtin_amdgcn_s_memtime();)
  // (everything below is issued behind the first group of operand loads: it is needed at epilogue time only)
  // the epilogue wave's bias / residual are requested up front (they would otherwise be a dependent
  // memory round trip at the very end of a microsecond-scale kernel)
  // MT >= 2: wave w < MT finishes row sub-tile w, four accumulator rows per lane.  MT == 1 (SPREAD): the one sub-tile's four
  // accumulator rows go to waves 0 .. 3 -- wave w finishes row w of every quad (rows 4 kq + w), one epilogue and one store per
  // lane, instead of four epilogues in sequence on wave 0 while the other waves idle.  Same operands, same order, per element.
  constexpr bool SPREAD = MT == 1;
  constexpr int ER = SPREAD ? 1 : 4;   // accumulator rows a lane finishes
  static_assert(NW >= 4, "the spread epilogue needs four waves");
  const int ep_mt = SPREAD ? 0 : wave;
  const int ep_r0 = SPREAD ? wave : 0;   // (wave-uniform) the first of them
  const bool is_ep = SPREAD ? (NW == 4 || wave < 4) : wave < MT;
  const int ep_n = n0 + col;
  float bias0 = 0.f, bias1 = 0.f, wsum0 = 0.f, wsum1 = 0.f, wbeta0 = 0.f, wbeta1 = 0.f, res[ER];
#pragma unroll
  for (int r = 0; r < ER; ++r) res[r] = 0.f;
  if (is_ep && ep_n < Nout) {
    if (p.bias) {
      bias0 = p.bias[ep_n];
      if (GLU) bias1 = p.bias[ep_n + Nout];
    }
    if (LN == LN_EPI) {
      wsum0 = p.ln_wsum[ep_n];
      if (GLU) wsum1 = p.ln_wsum[ep_n + Nout];
      if (p.mask_in) {
        wbeta0 = p.ln_wbeta[ep_n];
        if (GLU) wbeta1 = p.ln_wbeta[ep_n + Nout];
      }
    }
    if (p.resid) {
#pragma unroll
      for (int r = 0; r < ER; ++r) {
        const int m = min(m0 + 16 * ep_mt + 4 * kq + ep_r0 + r, p.M - 1);
        res[r] = p.resid[(size_t)m * p.ldr + ep_n];
      }
    }
  }
  // padded frames (masked_fill(0) before / after the layer, masked_fill_kernel.cu:27-54), for the rows this lane finishes.  An
  // input-masked row has a zero A row, i.e. a zero accumulator: the epilogue writes that instead of zeroing the A fragments in
  // front of every MFMA (a select + hazard nop per MFMA on the critical path of a one-tile wave).
  // MT == 1: only the REQUEST for the utterance's length stands here, behind the operand group like bias and residual, and
  // `frame >= length` is formed in the epilogue.  Resolved here, each row was a memory round trip of its own in front of the
  // epilogue wave's first MFMA, and the first of them drained the whole operand group.
  // MT >= 2: four lengths held across the MFMAs cost those forms a wave per SIMD; they ask for the four together and resolve
  // them here, one wait instead of four.
  int pad_len = 0;
  bool pad4[4] = {false, false, false, false};
  if (is_ep && (p.mask_in || p.mask_out)) {
    if (SPREAD) {
      pad_len = gemm_row_len_request(p, min(m0 + 4 * kq + ep_r0, p.M - 1));
    } else {
      int len4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) len4[r] = gemm_row_len_request(p, min(m0 + 16 * ep_mt + 4 * kq + r, p.M - 1));
#pragma unroll
      for (int r = 0; r < 4; ++r) pad4[r] = gemm_row_frame(p, min(m0 + 16 * ep_mt + 4 * kq + r, p.M - 1)) >= len4[r];
    }
  }

  // ---- LN_PRO: row statistics (two-pass) + gamma/beta to LDS, while the first loads are in flight ----
  float a_mean[MT], a_rstd[MT];
  float* ln_out_row[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    a_mean[mt] = 0.f;
    a_rstd[mt] = 1.f;
    ln_out_row[mt] = nullptr;
  }
  if (LN == LN_PRO) {
    for (int k = threadIdx.x * 4; k < Kl; k += 256 * NW) {
      *reinterpret_cast<f32x4*>(&ln_g[k]) = ldg4(p.ln_gamma + k);
      *reinterpret_cast<f32x4*>(&ln_b[k]) = ldg4(p.ln_beta + k);
    }
    // one 16-lane row group per A row (4 rows per wave pass): 256 B of a row per load instruction
    const int q = lane >> 4, l16 = lane & 15;
    const int nj = (Kl + 63) >> 6;                     // float4 per lane per row (<= 16 -> rows up to 1024 wide)
    for (int c = 0; c < (RW + 3) / 4; ++c) {
      const int rloc = wave * RW + 4 * c + q;
      const bool row_on = (4 * c + q) < RW;
      f32x4 v[16];
      if (!(ACCI && c == 0)) load_stat_rows(c);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = 4 * (l16 + 16 * j);
        const f32x4 t = ln_v[j];
        const bool in = j < nj && k < Kl;
        v[j] = f32x4{in ? t[0] : 0.f, in ? t[1] : 0.f, in ? t[2] : 0.f, in ? t[3] : 0.f};
      }
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
      const float mean = group16_sum(sum) / (float)Kl;
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = 4 * (l16 + 16 * j);
        const float on = (j < nj && k < Kl) ? 1.f : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = (v[j][e] - mean) * on;
          sq += d * d;
        }
      }
      const float var = group16_sum(sq) / (float)Kl;
      if (row_on && l16 == 0) {
        stats[rloc][0] = mean;
        stats[rloc][1] = rsqrtf(var + p.ln_eps);
      }
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      a_mean[mt] = stats[16 * mt + col][0];
      a_rstd[mt] = stats[16 * mt + col][1];
      const int m = m0 + 16 * mt + col;
      if (p.ln_out != nullptr && n_tile == 0 && m < p.M) ln_out_row[mt] = p.ln_out + (size_t)m * p.ld_ln_out + 4 * kq;
    }
  }

  auto compute_group = [&](int g, int buf) {
#pragma unroll
    for (int i = I0; i < G; ++i) {
      const int s = wave + NW * (G * g + i);
      if (s < nsteps) {
        const int k = s << 4;
        const bool in_ln = k >= ln_k0;
        f32x4 g4, b4;
        if (LN == LN_PRO && in_ln) {
          g4 = *reinterpret_cast<const f32x4*>(&ln_g[(k - ln_k0) + 4 * kq]);
          b4 = *reinterpret_cast<const f32x4*>(&ln_b[(k - ln_k0) + 4 * kq]);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          f32x4 a = abuf[buf][i][mt];
          if (LN == LN_PRO && in_ln) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = (a[j] - a_mean[mt]) * a_rstd[mt] * g4[j] + b4[j];
            // (holding the normalised fragments and storing them behind the last MFMA, so that no store acknowledgement is waited
            //  for between MFMAs, was built for the ACCI form and measured: no shorter)
            if (ln_out_row[mt] != nullptr) stg4(ln_out_row[mt] + (k - ln_k0), a);
          }
          if (LN == LN_EPI && in_ln) {
            s1[mt] += (a[0] + a[1]) + (a[2] + a[3]);
            s2[mt] += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
          }
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if (DUAL) {       // two independent accumulation chains (k even / odd inside the step): the fp32 MFMA has a 40-cycle
              //                 dependent latency against a 32-cycle issue, and a one-tile wave has nothing else to interleave
#pragma unroll
              for (int j = 0; j < 4; j += 2) {
                acc[mt][t] = mfma16(a[j], wbuf[buf][i][t][j], acc[mt][t]);
                acc2[mt][t] = mfma16(a[j + 1], wbuf[buf][i][t][j + 1], acc2[mt][t]);
              }
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[mt][t] = mfma16(a[j], wbuf[buf][i][t][j], acc[mt][t]);
            }
          }
        }
      }
    }
  };

  M3_GDIAG(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); dg[3] = __builtin_amdgcn_s_memtime();)
  if (NBUF == 1) {
    compute_group(0, 0);
  } else {
    for (int g = 0; g < ngroups; g += 2) {
      if (g + 1 < ngroups) load_group(g + 1, NBUF - 1);
      compute_group(g, 0);
      if (g + 1 < ngroups) {
        if (g + 2 < ngroups) load_group(g + 2, 0);
        compute_group(g + 1, NBUF - 1);
      }
    }
  }

  if (DUAL) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[mt][t] += acc2[mt][t];
  }
  M3_GDIAG(asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); dg[4] = __builtin_amdgcn_s_memtime();)
  // ---- cross-wave K reduction through LDS, then epilogue (MT >= 2: wave w finishes row sub-tile w; MT == 1: accumulator row w) ----
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][mt * NT + t][r * 64 + lane] = acc[mt][t][r];
  if (LN == LN_EPI) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float a1 = s1[mt], a2 = s2[mt];           // fold the 4 k-quarters of this wave (lanes col, col+16, +32, +48)
      a1 += __shfl_xor(a1, 16, 64);
      a2 += __shfl_xor(a2, 16, 64);
      a1 += __shfl_xor(a1, 32, 64);
      a2 += __shfl_xor(a2, 32, 64);
      if (kq == 0) {
        rsum[wave][16 * mt + col][0] = a1;
        rsum[wave][16 * mt + col][1] = a2;
      }
    }
  }
  __syncthreads();
  M3_GDIAG(dg[5] = __builtin_amdgcn_s_memtime();)

  if (is_ep) {
    const int mt = ep_mt;
    float v[NT][ER];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < ER; ++r) {
        const int e = (ep_r0 + r) * 64 + lane;
        float sum = 0.f;   // fixed summation order over the K-split -> bitwise reproducible
#pragma unroll
        for (int w = 0; w < NW; w += 4)
          sum += (red[w][mt * NT + t][e] + red[w + 1][mt * NT + t][e]) + (red[w + 2][mt * NT + t][e] + red[w + 3][mt * NT + t][e]);
        v[t][r] = sum;
      }
    if (ep_n < Nout) {
#pragma unroll
      for (int r = 0; r < ER; ++r) {
        const int row = 16 * mt + 4 * kq + ep_r0 + r;
        const int m = m0 + row;
        if (m >= p.M) continue;
        float y0 = v[0][r], y1 = v[NT - 1][r];
        bool pad = pad4[r];
        if (SPREAD && (p.mask_in || p.mask_out)) pad = gemm_row_frame(p, m) >= pad_len;
        if (LN != LN_EPI && p.mask_in && pad) y0 = y1 = 0.f;      // zero A row -> zero accumulator
        float mean = 0.f, rstd = 1.f;
        if (LN == LN_EPI) {
          float t1 = 0.f, t2 = 0.f;
#pragma unroll
          for (int w = 0; w < NW; ++w) {
            t1 += rsum[w][row][0];
            t2 += rsum[w][row][1];
          }
          ln_mean_rstd(t1, t2, Kl, p.ln_eps, mean, rstd);
        }
        float y = gemm_epilogue<GLU, LN == LN_EPI>(y0, y1, bias0, bias1, wsum0, wsum1, wbeta0, wbeta1, mean, rstd, pad, res[r], p);
        // a deferred GLU's gate columns (uniform per work-group: sig_col0 is a multiple of 16): the value the GLU epilogue hands to
        // its sigmoid, through the same sigmoid
        if (!GLU && p.sig_col0 >= 0 && n0 >= p.sig_col0) y = sigmoidf(y);
        p.Y[(size_t)m * p.ldy + ep_n] = y;
      }
    }
  }
  M3_GDIAG(dg[6] = __builtin_amdgcn_s_memtime();
           asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
           dg[7] = __builtin_amdgcn_s_memtime();
           if (lane == 0 && wave == 0 && bid < 2048) {
             unsigned long long* o = g_gemm_dbg + (size_t)bid * 8;
             for (int i = 0; i < 8; ++i) o[i] = dg[i];
             // where the work-group ran: HW_REG_HW_ID (id 4) and HW_REG_XCC_ID (id 20), packed above the last stamp's low 40 bits
             const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
             o[7] = (dg[7] & 0xffffffffffull) | ((unsigned long long)(hw & 0xffff) << 40) | ((unsigned long long)(xcc & 0xf) << 56);
           })
}

// Waves per SIMD an instantiation has to keep (the second argument of __launch_bounds__; 1 asks for nothing).  The two forms
// named here came out two VGPRs above the 96 that five waves allow, with no value more to hold than their neighbours, which fit
// (register allocation, not need): asked for, they fit as well, with no scratch.
constexpr int gemm_f32_min_waves(int MT, bool GLU, int NW, bool CONV, int LN, int NBUF, bool WF, bool dual) {
  return (MT == 1 && !GLU && NW == 8 && LN == LN_NONE && NBUF == 1 && ((dual && WF) || (!dual && CONV))) ? 5 : 1;
}

template <int MT, bool GLU, int NW, bool CONV, int LN, int NBUF, bool ACCI = false, bool WF = false>
__global__ __launch_bounds__(64 * NW, gemm_f32_min_waves(MT, GLU, NW, CONV, LN, NBUF, WF, false)) void gemm_f32_kernel(const GemmParams p) {
  gemm_f32_body<MT, GLU, NW, CONV, LN, NBUF, ACCI, WF>(p, (int)blockIdx.x);
}

// The A half of the concat GEMMs gemm_f32_kernel<1, false, NW, false, LN_PRO, 1, true> finishes, for several weight matrices over
// the same A rows (the routers of all main blocks: the embedding is final before block 0's and none of them changes it).
// Work-group (tile, layer), wave w: exactly the K-steps w, w + NW, ... < K1 / 16 of gemm_f32_body, the same operand fragments, the
// same two MFMA chains in the same order; the pair goes to memory as it stands, no reduction.
struct RouterPrefixArgs {
  const float* A; int lda; int M, N, K;            // K: row stride of the weights (both halves); the A half is columns [0, K / 2)
  int n_tiles, m_tiles, xcd_swizzle;
  const int32_t* m_dev;
  float* prefix; long layer_floats; int layer0;
  const float* w[kRouterPrefixMaxLayers];
};
template <int NW>
__global__ __launch_bounds__(64 * NW) void router_embed_prefix_kernel(const RouterPrefixArgs a) {
  constexpr int H = gemm_group_steps(1, 1, NW) / 2;   // K-steps per wave
  asm volatile("" ::"s"(a.A), "s"(a.lda), "s"(a.M), "s"(a.N), "s"(a.K), "s"(a.n_tiles), "s"(a.m_tiles), "s"(a.xcd_swizzle), "s"(a.m_dev),
               "s"(a.prefix), "s"(a.layer_floats), "s"(a.layer0));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int layer = a.layer0 + (int)blockIdx.y;
  int n_tile, m_tile;
  {
    const int id = (int)blockIdx.x;
    if (a.xcd_swizzle) {
      const int j = id >> 3;
      m_tile = j % a.m_tiles;
      n_tile = (j / a.m_tiles) * 8 + (id & 7);
    } else {
      n_tile = id % a.n_tiles;
      m_tile = id / a.n_tiles;
    }
  }
  const int n0 = n_tile * 16, m0 = m_tile * 16;
  if (a.m_dev != nullptr && m0 > *a.m_dev) return;   // (the consumer's tile exits the same way)
  const float* arow = a.A + (size_t)min(m0 + col, a.M - 1) * a.lda + 4 * kq;
  const float* wrow = a.w[layer] + (size_t)min(n0 + col, a.N - 1) * a.K + 4 * kq;
  f32x4 wb[H], ab[H];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const int k = (wave + NW * i) << 4;
    wb[i] = ldg4_w(wrow + k);
    ab[i] = ldg4(arow + k);
  }
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f}, acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < H; ++i)
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
      acc = mfma16(ab[i][j], wb[i][j], acc);
      acc2 = mfma16(ab[i][j + 1], wb[i][j + 1], acc2);
    }
  float* o = a.prefix + (size_t)layer * a.layer_floats + ((size_t)((m_tile * a.n_tiles + n_tile) * NW + wave) * 2) * 256 + 4 * lane;
  stg4(o, acc);
  stg4(o + 256, acc2);
}

size_t router_prefix_floats(const GemmPlan& plan) { return (size_t)plan.m_tiles * plan.n_tiles * plan.nw * 2 * 256; }

int launch_router_embed_prefix(const GemmPlan& plan, const GemmParams& p, const float* const* w, int layer0, int n_layers, float* prefix,
                               hipStream_t stream) {
  M3_REQUIRE(plan.launches == 1 && plan.kernel == GemmKernel::SkinnyF32 && p.acc_init != nullptr && (plan.nw == 4 || plan.nw == 8),
             "router prefix: the consumer's plan does not take an accumulator prefix");
  M3_REQUIRE(layer0 >= 0 && n_layers > 0 && layer0 + n_layers <= kRouterPrefixMaxLayers && prefix != nullptr, "router prefix: bad layer range");
  RouterPrefixArgs a;
  a.A = p.A; a.lda = p.lda; a.M = p.M; a.N = p.N; a.K = p.K;
  a.n_tiles = plan.n_tiles; a.m_tiles = plan.m_tiles; a.xcd_swizzle = plan.xcd_swizzle;
  a.m_dev = p.m_dev; a.prefix = prefix; a.layer_floats = (long)router_prefix_floats(plan); a.layer0 = layer0;
  for (int l = 0; l < kRouterPrefixMaxLayers; ++l) a.w[l] = (l >= layer0 && l < layer0 + n_layers) ? w[l] : nullptr;
  const dim3 grid(plan.n_tiles * plan.m_tiles, n_layers);
  if (plan.nw == 8) hipLaunchKernelGGL((router_embed_prefix_kernel<8>), grid, dim3(512), 0, stream, a);
  else hipLaunchKernelGGL((router_embed_prefix_kernel<4>), grid, dim3(256), 0, stream, a);
  M3_LAUNCH_CHECK();
  return 0;
}
// (the second problem's work-group ids start at a multiple of 8, so that "id % 8 = XCD" holds for its XCD-aware tile order too)
template <int MT, bool GLU, int NW, int LN, bool WF = false>
__global__ __launch_bounds__(64 * NW, gemm_f32_min_waves(MT, GLU, NW, false, LN, 1, WF, true)) void gemm_f32_dual_kernel(const GemmParams p0, const GemmParams p1, const int n0) {
  if ((int)blockIdx.x < n0) {
    if ((int)blockIdx.x < p0.n_tiles * p0.m_tiles) gemm_f32_body<MT, GLU, NW, false, LN, 1, false, WF>(p0, (int)blockIdx.x);
  } else {
    gemm_f32_body<MT, GLU, NW, false, LN, 1, false, WF>(p1, (int)blockIdx.x - n0);
  }
}

// the fields of the parameter block the skinny fp32 launchers fill: the plan's tile order, the multipliers of its divisors, one_run
static void gemm_fill_tiles(GemmParams& p, const GemmPlan& plan) {
  p.n_tiles = plan.n_tiles; p.m_tiles = plan.m_tiles; p.xcd_swizzle = plan.xcd_swizzle;
  p.div_m_tiles = gemm_div(plan.m_tiles);
  p.div_n_tiles = gemm_div(plan.n_tiles);
  p.div_rpb = gemm_div(p.rows_per_batch > 0 ? p.rows_per_batch : 1);
  p.one_run = p.rows_per_batch >= p.M ? 1 : 0;
}

// two independent problems of one instantiation in ONE launch (gemm_dual_fusable holds for the two records)
int launch_gemm_f32_dual(const GemmLaunch& a, const GemmLaunch& b, hipStream_t stream) {
  M3_REQUIRE(gemm_dual_fusable(a, b), "gemm dual: the two problems do not share an instantiation");
  GemmParams q[2] = {a.p, b.p};
  const GemmPlan& pa = a.plan;
  const GemmPlan* const plans[2] = {&a.plan, &b.plan};
  for (int i = 0; i < 2; ++i) gemm_fill_tiles(q[i], *plans[i]);
  const int n0 = (int)align_up((size_t)q[0].n_tiles * q[0].m_tiles, 8);
  dim3 grid(n0 + q[1].n_tiles * q[1].m_tiles);
#define M3_DUAL(GLU_, NW_, LN_)                                                                                             \
  do {                                                                                                                      \
    if (q[0].w_frag) hipLaunchKernelGGL((gemm_f32_dual_kernel<1, GLU_, NW_, LN_, true>), grid, dim3(64 * NW_), 0, stream, q[0], q[1], n0); \
    else hipLaunchKernelGGL((gemm_f32_dual_kernel<1, GLU_, NW_, LN_>), grid, dim3(64 * NW_), 0, stream, q[0], q[1], n0);    \
  } while (0)
  if (pa.glu) {
    if (pa.nw == 8) { if (pa.ln == LN_EPI) M3_DUAL(true, 8, LN_EPI); else M3_DUAL(true, 8, LN_NONE); }
    else { if (pa.ln == LN_EPI) M3_DUAL(true, 4, LN_EPI); else M3_DUAL(true, 4, LN_NONE); }
  } else {
    if (pa.nw == 8) { if (pa.ln == LN_EPI) M3_DUAL(false, 8, LN_EPI); else M3_DUAL(false, 8, LN_NONE); }
    else { if (pa.ln == LN_EPI) M3_DUAL(false, 4, LN_EPI); else M3_DUAL(false, 4, LN_NONE); }
  }
#undef M3_DUAL
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_gemm_f32_skinny(const GemmPlan& plan, const GemmParams& pin, hipStream_t stream) {
  GemmParams p = pin;
  gemm_fill_tiles(p, plan);
  dim3 grid(p.n_tiles * p.m_tiles);
  const int mt = plan.mt, nw = plan.nw, ln = plan.ln;
  if (p.acc_init != nullptr) {        // (plan_gemm: 16-row tiles, 4 / 8 waves, one load group, affine LayerNorm on the A2 half)
    if (nw == 8) hipLaunchKernelGGL((gemm_f32_kernel<1, false, 8, false, LN_PRO, 1, true>), grid, dim3(512), 0, stream, p);
    else hipLaunchKernelGGL((gemm_f32_kernel<1, false, 4, false, LN_PRO, 1, true>), grid, dim3(256), 0, stream, p);
    M3_LAUNCH_CHECK();
    return 0;
  }

#define M3_GEMM_LAUNCH(MT_, GLU_, NW_, CONV_, LN_)                                                              \
  do {                                                                                                          \
    constexpr bool kWf = !(CONV_);   /* (the plan: fragment-ordered W never comes with an implicit conv) */      \
    if (p.w_frag && plan.nbuf == 1)                                                                              \
      hipLaunchKernelGGL((gemm_f32_kernel<MT_, GLU_, NW_, CONV_, LN_, 1, false, kWf>), grid, dim3(64 * NW_), 0, stream, p); \
    else if (p.w_frag)                                                                                           \
      hipLaunchKernelGGL((gemm_f32_kernel<MT_, GLU_, NW_, CONV_, LN_, 2, false, kWf>), grid, dim3(64 * NW_), 0, stream, p); \
    else if (plan.nbuf == 1)                                                                                    \
      hipLaunchKernelGGL((gemm_f32_kernel<MT_, GLU_, NW_, CONV_, LN_, 1>), grid, dim3(64 * NW_), 0, stream, p); \
    else                                                                                                        \
      hipLaunchKernelGGL((gemm_f32_kernel<MT_, GLU_, NW_, CONV_, LN_, 2>), grid, dim3(64 * NW_), 0, stream, p); \
  } while (0)
#define M3_GEMM_MT(GLU_, NW_, CONV_, LN_)                                                              \
  do {                                                                                                 \
    if (mt == 1) M3_GEMM_LAUNCH(1, GLU_, NW_, CONV_, LN_);                                             \
    else if (mt == 2) M3_GEMM_LAUNCH(2, GLU_, NW_, CONV_, LN_);                                        \
    else M3_GEMM_LAUNCH(4, GLU_, NW_, CONV_, LN_);                                                     \
  } while (0)
#define M3_GEMM_LN(GLU_, NW_)                                                                          \
  do {                                                                                                 \
    if (ln == LN_EPI) M3_GEMM_MT(GLU_, NW_, false, LN_EPI);                                            \
    else if (ln == LN_PRO) M3_GEMM_MT(GLU_, NW_, false, LN_PRO);                                       \
    else M3_GEMM_MT(GLU_, NW_, false, LN_NONE);                                                        \
  } while (0)
  if (plan.conv) {                  // implicit 3x3 conv: no GLU, no LayerNorm
    if (nw == 16) M3_GEMM_MT(false, 16, true, LN_NONE); else if (nw == 8) M3_GEMM_MT(false, 8, true, LN_NONE);
    else M3_GEMM_MT(false, 4, true, LN_NONE);
  } else if (nw == 16) {            // K >= 2048: plain only
    M3_GEMM_MT(false, 16, false, LN_NONE);
  } else if (plan.glu) {
    if (nw == 8) M3_GEMM_LN(true, 8); else M3_GEMM_LN(true, 4);
  } else {
    if (nw == 8) M3_GEMM_LN(false, 8); else M3_GEMM_LN(false, 4);
  }
#undef M3_GEMM_LN
#undef M3_GEMM_MT
#undef M3_GEMM_LAUNCH
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3

#ifdef M3_GEMM_DIAG
extern "C" int m3_debug_gemm_read(void* dst, size_t bytes) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(m3::g_gemm_dbg), bytes < sizeof(m3::g_gemm_dbg) ? bytes : sizeof(m3::g_gemm_dbg));
}
#endif
