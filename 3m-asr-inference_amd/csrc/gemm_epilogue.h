// The dense GEMMs' epilogue, written once (device only; every kernel of the family includes it).  The floating-point
// operations stand in the order every kernel had them, and the build has -ffp-contract=off: same source order, same bits.
#pragma once
#include "common.h"
#include "kernels.h"

namespace m3 {

// masked_fill (masked_fill_kernel.cu:27-54): row m is frame m % rows_per_batch of utterance m / rows_per_batch; padded past row_len
__device__ __forceinline__ bool gemm_row_padded(const GemmParams& p, int m) {
  return (m % p.rows_per_batch) >= p.row_len[m / p.rows_per_batch];
}

// x / d by the host's multiplier (kernels.h GemmDiv): exact for 0 <= x < 2^31
__device__ __forceinline__ int gemm_div_by(int x, const GemmDiv& d) { return (int)(((unsigned long long)(unsigned)x * d.mul) >> d.shift); }

// The same test in two halves, for a kernel that must not wait for row_len where it asks for it (gemm_f32_body): the request
// up front (the utterance's length, in flight), the comparison `gemm_row_frame(p, m) >= len` where the row is finished.
// one_run (rows_per_batch >= M, set by the launcher): utterance 0, frame == m.
__device__ __forceinline__ int gemm_row_len_request(const GemmParams& p, int m) {
  return p.row_len[p.one_run ? 0 : gemm_div_by(m, p.div_rpb)];
}
__device__ __forceinline__ int gemm_row_frame(const GemmParams& p, int m) {
  return p.one_run ? m : m - gemm_div_by(m, p.div_rpb) * p.rows_per_batch;
}

// folded LayerNorm: mean and 1 / std of a K-wide row from its sum and sum of squares
__device__ __forceinline__ void ln_mean_rstd(float sum, float sumsq, int K, float eps, float& mean, float& rstd) {
  mean = sum / (float)K;
  const float var = fmaxf(sumsq / (float)K - mean * mean, 0.f);
  rstd = rsqrtf(var + eps);
}

// sum over W = 8 / 16 / 32 consecutive lanes (aligned to W): DPP butterfly of the right width, one LDS-free shuffle for 32
template <int W>
__device__ __forceinline__ float lanes_sum(float v) {
  static_assert(W == 8 || W == 16 || W == 32, "8, 16 or 32 lanes");
  v += dpp_mov<0xB1>(v);    // xor 1
  v += dpp_mov<0x4E>(v);    // xor 2
  v += dpp_mov<0x141>(v);   // row_half_mirror: 8 lanes
  if (W >= 16) v += dpp_mov<0x140>(v);   // row_mirror: 16 lanes
  if (W == 32) v += __shfl_xor(v, 16, 64);
  return v;
}

// One output element: folded-LayerNorm correction, bias, GLU, ReLU / SiLU, output mask, alpha, residual.
// (y0, y1): the accumulator's value and gate column (y1 and the *1 constants: GLU only); pad: the row is a padded frame.
// An input-masked row under the folded LayerNorm (masked_fill(0) after the LayerNorm) contributes the plain bias only.
template <bool GLU, bool LN>
__device__ __forceinline__ float gemm_epilogue(float y0, float y1, float bias0, float bias1, float wsum0, float wsum1, float wbeta0,
                                               float wbeta1, float mean, float rstd, bool pad, float res, const GemmParams& p) {
  if (LN) {
    if (p.mask_in && pad) {
      y0 = -wbeta0;
      y1 = -wbeta1;
    } else {
      y0 = rstd * (y0 - mean * wsum0);
      y1 = rstd * (y1 - mean * wsum1);
    }
  }
  float y = y0 + bias0;
  if (GLU) y = y * sigmoidf(y1 + bias1);
  if (p.act == ACT_RELU) y = fmaxf(y, 0.f);
  if (p.act == ACT_SILU) y = silu(y);
  if (p.mask_out && pad) y = 0.f;
  y *= p.alpha;
  if (p.resid) y += res;
  return y;
}

}  // namespace m3
