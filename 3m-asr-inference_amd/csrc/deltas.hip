// Delta features in: Kaldi's DeltaFeatures (feat/feature-functions.cc, add-deltas) on the device: static
// frames (B, ., bins) -> static | delta | delta-delta, (order + 1) * bins columns per frame.
//
// Contract: scales_0 = [1], scales_i = conv(scales_{i-1}, [-W..W]) / sum_j j^2, so scales_i has 2 i W + 1 taps, and block i of
// output frame t is
//     y_i[t] = sum_{j = -iW..iW} scales_i[j] x[clamp(lead + t + j, 0, n_in - 1)].
// The clamp sits on the COMPOSITE filter's taps on the static frames: that is Kaldi's edge replication, and it is not what
// iterating a first-order delta with replicate padding gives in the first and last W frames.  `lead` counts frames in front
// that are context only, so the same rule serves the whole utterance (lead = 0, n_out = n_in) and a streaming window whose
// frames left and right of the produced ones are real history and lookahead.
//
// Layout: a work-group of 256 lanes owns DL_TILE = 32 consecutive output frames of one row.  It stages the DL_TILE + 2 R
// static frames its taps can reach (R = order * W <= 8; the clamp is applied here, to the frame index) in LDS, so memory is
// read once per element plus the halo, then lane l takes the items l, l + 256, ... of (frame, column quad) -- or (frame,
// column) on the scalar path, taken when bins % 4 != 0 or a stride or pointer is not a whole 16 bytes.  An item copies the
// static value out of LDS bit for bit and computes each delta block as ONE fp32 fma chain from 0 over the block's taps in
// ascending j.  No cross-lane step: a frame's bits depend on its taps and the table only, not on B, the tile, lead or the
// path, so a stream computed window by window equals the utterance computed at once.  ORDER and W are template arguments:
// the tap loops are fully unrolled and the table (a kernel argument, built on the HOST in float64 and rounded once) is read
// at constant offsets.
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace m3 {

namespace {

constexpr int DL_THREADS = 256, DL_TILE = 32, DL_MAX_R = DELTAS_MAX_CONTEXT, DL_ROW = 2 * DL_MAX_R + 1;

// scales_i[j] at s[i - 1][DL_MAX_R + j]; zero outside |j| <= i W
struct DeltaTable {
  float s[2][DL_ROW];
};

struct DeltaArgs {
  const float* feat;
  long ld_feat, bs_feat;
  int T_in;
  const int32_t* n_in;
  const int32_t* lead;
  const int32_t* n_out;
  int T_out, bins;
  float* out;
  long ld_out, bs_out;
  int32_t* out_len;
  int inplace;
};

template <int ORDER, int W, bool VEC>
__global__ __launch_bounds__(DL_THREADS) void add_deltas_kernel(const DeltaArgs a, const DeltaTable tab) {
  constexpr int R = ORDER * W, E = VEC ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) float dl_stage[];    // (DL_TILE + 2 R) rows of `pitch` floats
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile0 = blockIdx.x * DL_TILE;                             // < T_out
  const int tile_n = min(DL_TILE, a.T_out - tile0);
  const int bins = a.bins, Q = VEC ? bins / 4 : bins;                 // items per frame
  const int pitch = (bins + 3) & ~3;                                  // a row of the stage starts on 16 bytes
  const int n = min(max(a.n_in[b], 0), a.T_in);                       // static frames the row holds
  const int ld = a.lead ? min(max(a.lead[b], 0), n) : 0;
  const int want = min(min(max(a.n_out[b], 0), n - ld), a.T_out);
  if (a.out_len && blockIdx.x == 0 && tid == 0) a.out_len[b] = want;
  const int live = min(max(want - tile0, 0), tile_n);                 // frames of this tile that are computed; the rest are zeros
  const float* const frow = a.feat + (long)b * a.bs_feat;
  float* const orow = a.out + (long)b * a.bs_out + (long)tile0 * a.ld_out;

  if (live > 0) {                                                     // then n >= 1: the clamp has a frame to land on
    const int rows = live + 2 * R;
    for (int i = tid; i < rows * Q; i += DL_THREADS) {
      const int r = i / Q, q = i - r * Q;
      const int src = min(max(ld + tile0 + r - R, 0), n - 1);
      const float* const p = frow + (long)src * a.ld_feat + q * E;
      if (VEC)
        *reinterpret_cast<f32x4*>(dl_stage + r * pitch + q * 4) = ldg4(p);
      else
        dl_stage[r * pitch + q] = *p;
    }
  }
  __syncthreads();

  for (int i = tid; i < tile_n * Q; i += DL_THREADS) {
    const int t = i / Q, q = i - t * Q;
    float* const o = orow + (long)t * a.ld_out + q * E;
    float x[2 * R + 1][E], y[ORDER][E];
    if (t < live) {
#pragma unroll
      for (int j = 0; j <= 2 * R; ++j) {
        const float* const p = dl_stage + (t + j) * pitch + q * E;
        if (VEC) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
          for (int e = 0; e < E; ++e) x[j][e] = v[e];
        } else {
          x[j][0] = *p;
        }
      }
#pragma unroll
      for (int k = 1; k <= ORDER; ++k) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          float acc = 0.f;
#pragma unroll
          for (int j = -k * W; j <= k * W; ++j) acc = __fmaf_rn(tab.s[k - 1][DL_MAX_R + j], x[R + j][e], acc);
          y[k - 1][e] = acc;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        x[R][e] = 0.f;
#pragma unroll
        for (int k = 0; k < ORDER; ++k) y[k][e] = 0.f;
      }
    }
    if (VEC) {
      if (!a.inplace) stg4(o, f32x4{x[R][0], x[R][1], x[R][2], x[R][3]});
#pragma unroll
      for (int k = 0; k < ORDER; ++k) stg4(o + (k + 1) * bins, f32x4{y[k][0], y[k][1], y[k][2], y[k][3]});
    } else {
      if (!a.inplace) o[0] = x[R][0];
#pragma unroll
      for (int k = 0; k < ORDER; ++k) o[(k + 1) * bins] = y[k][0];
    }
  }
}

template <int ORDER, int W>
int launch_ow(const DeltaArgs& a, const DeltaTable& tab, int B, bool vec, hipStream_t stream) {
  const dim3 grid((unsigned)((a.T_out + DL_TILE - 1) / DL_TILE), (unsigned)B);
  const size_t lds = (size_t)(DL_TILE + 2 * ORDER * W) * ((a.bins + 3) & ~3) * sizeof(float);
  if (vec)
    hipLaunchKernelGGL((add_deltas_kernel<ORDER, W, true>), grid, dim3(DL_THREADS), lds, stream, a, tab);
  else
    hipLaunchKernelGGL((add_deltas_kernel<ORDER, W, false>), grid, dim3(DL_THREADS), lds, stream, a, tab);
  M3_LAUNCH_CHECK();
  return 0;
}

template <int ORDER>
int launch_o(const DeltaArgs& a, const DeltaTable& tab, int window, int B, bool vec, hipStream_t stream) {
  switch (window) {
    case 1: return launch_ow<ORDER, 1>(a, tab, B, vec, stream);
    case 2: return launch_ow<ORDER, 2>(a, tab, B, vec, stream);
    case 3: return launch_ow<ORDER, 3>(a, tab, B, vec, stream);
    default: return launch_ow<ORDER, 4>(a, tab, B, vec, stream);
  }
}

}  // namespace

int deltas_options_ok(int order, int window) {
  M3_REQUIRE(order >= 1 && order <= 2, "add_deltas: order=%d outside [1, 2]", order);
  M3_REQUIRE(window >= 1 && window <= 4, "add_deltas: window=%d outside [1, 4]", window);
  return 0;
}

// scales_0 .. scales_order in float64, rounded once: row i of `scales` ((order + 1) rows of 2 * DELTAS_MAX_CONTEXT + 1 floats)
// holds scales_i[j] at column DELTAS_MAX_CONTEXT + j and zeros elsewhere.
int deltas_tables_build(int order, int window, float* scales) {
  if (int rc = deltas_options_ok(order, window)) return rc;
  double s[3][DL_ROW];
  memset(s, 0, sizeof(s));
  s[0][DL_MAX_R] = 1.0;
  double norm = 0.0;
  for (int j = -window; j <= window; ++j) norm += (double)(j * j);
  for (int i = 1; i <= order; ++i)
    for (int k = -(i - 1) * window; k <= (i - 1) * window; ++k)
      for (int j = -window; j <= window; ++j) s[i][DL_MAX_R + k + j] += (double)j * s[i - 1][DL_MAX_R + k] / norm;
  for (int i = 0; i <= order; ++i)
    for (int c = 0; c < DL_ROW; ++c) scales[i * DL_ROW + c] = (float)s[i][c];
  return 0;
}

int launch_add_deltas(const float* feat, long ld_feat, long bs_feat, int T_in, const int32_t* n_in, const int32_t* lead,
                      const int32_t* n_out, int B, int T_out, int bins, int order, int window, float* out, long ld_out,
                      long bs_out, int32_t* out_len, hipStream_t stream) {
  if (int rc = deltas_options_ok(order, window)) return rc;
  if (B == 0 || T_out == 0) return 0;
  float scales[3 * DL_ROW];
  if (int rc = deltas_tables_build(order, window, scales)) return rc;
  DeltaTable tab;
  memset(&tab, 0, sizeof(tab));
  for (int i = 1; i <= order; ++i) memcpy(tab.s[i - 1], scales + i * DL_ROW, sizeof(tab.s[0]));
  DeltaArgs a;
  a.feat = feat;
  a.ld_feat = ld_feat;
  a.bs_feat = bs_feat;
  a.T_in = T_in;
  a.n_in = n_in;
  a.lead = lead;
  a.n_out = n_out;
  a.T_out = T_out;
  a.bins = bins;
  a.out = out;
  a.ld_out = ld_out;
  a.bs_out = bs_out;
  a.out_len = out_len;
  a.inplace = out == feat;
  const bool vec = bins % 4 == 0 && ld_feat % 4 == 0 && bs_feat % 4 == 0 && ld_out % 4 == 0 && bs_out % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(feat) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  return order == 1 ? launch_o<1>(a, tab, window, B, vec, stream) : launch_o<2>(a, tab, window, B, vec, stream);
}

}  // namespace m3
