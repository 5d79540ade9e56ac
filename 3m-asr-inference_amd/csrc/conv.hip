// Convolution pieces of the hot path that are not GEMM-shaped (fp32, channel-last).
//
//   dwconv_ln_silu_kernel : ConvolutionModule's depthwise Conv1d(k=15, groups=C) + LayerNorm(eps 1e-5)
//                           + SiLU (trainer_3m_fix/layer/convolution.py:134-152; TRT conv
//                           torch_network_helper.py:199-225, LayerNorm plugin, SiLU :827-841) fused,
//                           on (B,T',C) rows so the two "use_layer_norm_trans" shuffles disappear.
//   conv1_relu_kernel     : first subsampling Conv2d(1,C,3,stride 2) + ReLU
//                           (trainer_3m_fix/layer/subsampling.py:113-114) writing channel-last
//                           (B,T1,F1,C) so the second conv becomes an implicit GEMM (gemm.hip).
//   depthwise_conv1d_nct  : plain (B,C,T) depthwise conv for the op-by-op network_helper path.
#include "common.h"
#include "kernels.h"

namespace m3 {

// z, out: [B*T][D]; w_kc: [K][D] (repacked from (D,1,K)).  One workgroup per frame, one float4 of
// channels per thread (D/4 threads): all K taps (z rows t-pad..t+pad and their weights) are loaded
// before the first FMA, so a frame costs one memory round trip; edge taps read a clamped row and are
// multiplied by 0 (= the conv's zero padding).  LayerNorm statistics go through a small LDS tree.
//
// Causal form (convolution.py:43-49,118-123: lorder = K - 1 frames are padded on the LEFT of the module's input, in front of
// pointwise_conv1, and the depthwise conv runs without padding): out[t] = sum_k w[k] z[t - (K-1) + k], no taps to the right.
// The K-1 frames left of frame 0 are not zeros at the depthwise conv's input: pointwise_conv1 + GLU turn a zero frame into
// the constant row GLU(bias).  `cs.left` supplies them: one broadcast row ("left_fill" of the plan; full-utterance forward),
// or, chunk by chunk, the last K-1 frames of the previous chunk's z from the streaming state (a ping-pong pair selected by
// the parity of the device-side chunk counter; the work-groups past the B*T frames write the other half: the new cache =
// the last K-1 frames of [cache | z[0 : len)], cat_split_cache_kernel.cu:30-55's contract on frames instead of elements).
struct DwCausal {
  int causal = 0;                          // 1: lorder = K - 1, no right taps
  const float* left = nullptr;             // causal: frames t < 0.  left_t_stride 0: one row [D] for every t < 0 and utterance
  long left_b_stride = 0; int left_t_stride = 0;
  const int32_t* step = nullptr;           // streaming: device-side chunk counter; `left` then is the [2][B][K-1][D] ping-pong pair
  long half = 0;                           // floats in one half of the pair
  const int32_t* chunk_len = nullptr;      // streaming: valid frames of this chunk per utterance
  int max_chunks = 0;                      // streaming in slot mode (SLOTS kernels only): `step` is [B], one counter per utterance
};

// CAUSAL is a template parameter: the symmetric form is the round-3 kernel instruction for instruction (making it a run-time
// field of one kernel cost 4.9 -> 8.3 us per launch at B = 1: a pointer select in front of every tap load).
// (the body as a device function of the work-group's row: dwconv_ln_silu_dual_kernel runs two independent problems in one launch,
//  see gemm.hip / engine.hip "horizontal fusion")
// SLOTS is a template parameter for the same reason: the lockstep streaming form reads ONE counter, slot mode utterance b's own
// (cs.step[b]); a slot that is not live in this chunk (stream_slot_live) leaves its cache pair alone.
// GLU_IN (symmetric form only): z is the pointwise_conv1 GEMM's raw [rows][ldz] output, value columns [0, D) | gate columns
// [D, 2 D) (bias added, no GLU): every tap is value * sigmoid(gate) as it is loaded -- the operation, and the operands, the GEMM's
// GLU epilogue has (gemm_epilogue.h), so the taps hold the same bits.  The GEMM in front then is the plain one-column-tile form:
// twice the work-groups, 64 instead of 96 KB of operands through each CU.  All 2 K row loads still precede the first use.
// GLU_IN = 2: the gate columns hold sigmoid(gate) already -- the GEMM's epilogue formed it once per element (GemmParams::sig_col0)
// where this kernel would form it in each of the K work-groups whose taps touch the row.  Every tap is value * gate', the
// multiply GLU_IN = 1 ends with, on the same operands: the same bits, and no exp / divide chain behind the last load.
template <int KT, bool CAUSAL, bool SLOTS = false, int GLU_IN = 0>
__device__ __forceinline__ void dwconv_ln_silu_body(const float* __restrict__ z, const float* __restrict__ w_kc,
                                                    const float* __restrict__ bias, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float eps, int T, int D, int K,
                                                    float* __restrict__ out, int out_bf16, const int32_t* __restrict__ pad_of,
                                                    const int32_t* __restrict__ row0, const int32_t* __restrict__ row_len,
                                                    int n_rows, const DwCausal& cs, const int row, const int ldz = 0) {
  static_assert(!GLU_IN || (!CAUSAL && !SLOTS), "GLU on load: the symmetric conv only");
  __shared__ float red[2][16];
  // one batch of kernel-argument loads instead of one per first use (see gemm.hip: ~6 dependent s_load rounds otherwise)
  asm volatile("" ::"s"(z), "s"(w_kc), "s"(bias), "s"(gamma), "s"(beta), "s"(eps), "s"(T), "s"(D), "s"(K), "s"(out), "s"(out_bf16),
               "s"(pad_of), "s"(row0), "s"(row_len), "s"(n_rows));
  const int c = threadIdx.x * 4;
  const bool live = c < D;
  const size_t zs = GLU_IN ? (size_t)ldz : (size_t)D;   // row stride of z
  const float* leftp = cs.left;
  if (CAUSAL && cs.step != nullptr) {                         // streaming: read half (step & 1), write the other one
    int par;
    if (SLOTS) {                                    // the parity of this row's slot; only a parity is taken from the counter
      const int sb = row >= n_rows ? (row - n_rows) / (K - 1) : row / T;
      const int pos = cs.step[sb];
      if (row >= n_rows && !stream_slot_live(cs.chunk_len[sb], pos, cs.max_chunks)) return;
      par = pos & 1;
    } else {
      par = *cs.step & 1;
    }
    leftp = cs.left + (size_t)par * cs.half;
    if (row >= n_rows) {                            // cache update: row i of utterance b <- frame i + len of [cache | z]
      const int i = row - n_rows, b = i / (K - 1), ci = i - b * (K - 1);
      const int s = ci + min(max(cs.chunk_len[b], 0), T);
      const float* src = s < K - 1 ? leftp + (size_t)b * cs.left_b_stride + (size_t)s * cs.left_t_stride
                                   : z + ((size_t)b * T + (s - (K - 1))) * D;
      float* dst = const_cast<float*>(cs.left) + (size_t)(par ^ 1) * cs.half + (size_t)b * cs.left_b_stride + (size_t)ci * cs.left_t_stride;
      if (live) stg4(dst + c, ldg4(src + c));
      return;
    }
  }
  // padded rows: row = b T + t.  Packed rows (pad_of != null): row p is frame pad_of[p] = b T + t of the padded layout
  // (-1 past the last packed row P); utterance b owns rows [row0[b], row0[b] + len).  The reference runs the conv on the
  // padded batch, where the frames len <= tt < T hold the constant row pointwise_conv1 produces from a zeroed input
  // (masked_fill before the conv module, convolution.py:101-104): the packed layout keeps one copy of it at row P
  // (written by the pw1 GEMM with rows >= P masked), and tt < 0 or tt >= T are the conv's zero padding as before.
  int b = row / T, t = row % T, len = T;
  size_t r0 = (size_t)b * T, rpad = 0;
  if (pad_of != nullptr) {
    const int pr = pad_of[row];
    if (pr < 0) return;
    b = pr / T;
    t = pr - b * T;
    len = row_len[b];
    r0 = (size_t)row0[b];
    rpad = (size_t)row0[n_rows / T];                  // P = row0[B]
  }
  const int pad = CAUSAL ? K - 1 : (K - 1) / 2;
  if (CAUSAL) leftp += (size_t)b * cs.left_b_stride + (size_t)(K - 1) * cs.left_t_stride;   // frame tt < 0 is leftp + tt * left_t_stride
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (live) {
    v = ldg4(bias + c);
    for (int k0 = 0; k0 < K; k0 += KT) {
      f32x4 zz[KT], ww[KT], gg[GLU_IN ? KT : 1];
      float on[KT];
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        const int k = min(k0 + kk, K - 1);
        const int tt = t + k - pad;
        const int tc = min(max(tt, 0), T - 1);
        const float* src = z + (tc < len ? r0 + tc : rpad) * zs;
        if (CAUSAL) {                                 // no taps to the right; frames left of the utterance come from `left`
          on[kk] = (k0 + kk < K) ? 1.f : 0.f;
          if (tt < 0) src = leftp + (long)tt * cs.left_t_stride;
        } else {
          on[kk] = (k0 + kk < K && tt >= 0 && tt < T) ? 1.f : 0.f;
        }
        zz[kk] = ldg4(src + c);
        if (GLU_IN) gg[kk] = ldg4(src + D + c);
        ww[kk] = ldg4(w_kc + (size_t)k * D + c);
      }
      if (GLU_IN == 2) {
        // (as below: every tap is requested before the first is used -- one round trip for the 3 K loads, not one per few taps)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KT; ++kk)
#pragma unroll
          for (int j = 0; j < 4; ++j) zz[kk][j] = zz[kk][j] * gg[kk][j];
      }
      if (GLU_IN == 1) {
        // all 3 K loads are issued before the first sigmoid: the 60 exp + divide of a thread would otherwise be scheduled between
        // them and the taps would arrive in six or seven dependent round trips instead of one
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KT; ++kk)
#pragma unroll
          for (int j = 0; j < 4; ++j) zz[kk][j] = zz[kk][j] * sigmoidf(gg[kk][j]);
      }
#pragma unroll
      for (int kk = 0; kk < KT; ++kk)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(zz[kk][j] * on[kk], ww[kk][j], v[j]);
    }
  }
  if (gamma != nullptr) {
    float s = live ? (v[0] + v[1]) + (v[2] + v[3]) : 0.f;
    s = wave_sum(s);
    if (lane == 0) red[0][wave] = s;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < nwaves; ++w) tot += red[0][w];
    const float mean = tot / (float)D;
    float q = 0.f;
    if (live) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[j] - mean;
        q += d * d;
      }
    }
    q = wave_sum(q);
    if (lane == 0) red[1][wave] = q;
    __syncthreads();
    float qt = 0.f;
    for (int w = 0; w < nwaves; ++w) qt += red[1][w];
    const float rstd = rsqrtf(qt / (float)D + eps);
    if (live) {
      const f32x4 g = ldg4(gamma + c), be = ldg4(beta + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (v[j] - mean) * rstd * g[j] + be[j];
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = silu(v[j]);
    if (out_bf16) {
      bf16x4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = (bf16_t)v[j];
      *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(out) + (size_t)row * D + c) = h;
    } else {
      stg4(out + (size_t)row * D + c, v);
    }
  }
}

// One record per problem, filled by dwconv_pack: the single kernel takes one, the dual kernel two.
struct DwKernArgs {
  const float *z, *w_kc, *bias, *gamma, *beta; float eps; int T, D, K; float* out; int out_bf16;
  const int32_t *pad_of, *row0, *row_len; int n_rows; DwCausal cs; int ldz;
  int slots, glu_in, threads, grid;   // the launch: instantiation (with cs.causal and K), block, work-groups
};
#define M3_DW_SPREAD(a) a.z, a.w_kc, a.bias, a.gamma, a.beta, a.eps, a.T, a.D, a.K, a.out, a.out_bf16, a.pad_of, a.row0, a.row_len, a.n_rows, a.cs
// (GLU_IN holds 2 K row fragments + K weight fragments per thread: 256 threads (D <= 1024) leave a wave the registers for them)
template <int KT, bool CAUSAL, bool SLOTS = false, int GLU_IN = 0>
__global__ __launch_bounds__(GLU_IN ? 256 : 1024) void dwconv_ln_silu_kernel(const DwKernArgs a) {
  dwconv_ln_silu_body<KT, CAUSAL, SLOTS, GLU_IN>(M3_DW_SPREAD(a), (int)blockIdx.x, a.ldz);
}
template <int KT, bool CAUSAL, int GLU_IN = 0>
__global__ __launch_bounds__(GLU_IN ? 256 : 1024) void dwconv_ln_silu_dual_kernel(const DwKernArgs a, const DwKernArgs b) {
  if ((int)blockIdx.x < a.n_rows) dwconv_ln_silu_body<KT, CAUSAL, false, GLU_IN>(M3_DW_SPREAD(a), (int)blockIdx.x, a.ldz);
  else dwconv_ln_silu_body<KT, CAUSAL, false, GLU_IN>(M3_DW_SPREAD(b), (int)blockIdx.x - a.n_rows, b.ldz);
}
#undef M3_DW_SPREAD

bool dwconv_glu_in_supports(int D, int K, bool causal_or_stream, int out_bf16, int ldz) {
  return !causal_or_stream && !out_bf16 && (K & 1) == 1 && K <= 15 && D >= 256 && D <= 1024 && (D & 3) == 0 && ldz >= 2 * D && (ldz & 3) == 0;
}
static bool dwconv_causal(const DwArgs& a) { return a.streaming || a.causal_left_fill != nullptr; }
static int check_dwconv(const DwArgs& a, bool say = true) {
  const bool causal = dwconv_causal(a);
  M3_REQUIRE_SAY(say, !a.streaming || (a.cache_pair && a.step && a.chunk_len), "dwconv (stream): null state");
  M3_REQUIRE_SAY(say, !a.glu_ldz || a.causal_left_fill == nullptr, "dwconv (GLU on load): the symmetric conv only");
  M3_REQUIRE_SAY(say, a.glu_ldz == 0 || dwconv_glu_in_supports(a.D, a.K, causal, a.out_bf16, a.glu_ldz),
                 "dwconv (GLU on load): needs the symmetric fp32 conv, K <= 15, 256 <= channels <= 1024, ldz=%d a multiple of 4 and >= %d", a.glu_ldz, 2 * a.D);
  M3_REQUIRE_SAY(say, !a.streaming || a.slot_max_chunks != 0, "dwconv (slot mode): needs the streaming causal form");
  M3_REQUIRE_SAY(say, (a.D & 3) == 0 && a.D <= 4096, "dwconv: channels=%d must be a multiple of 4 (<=4096)", a.D);
  M3_REQUIRE_SAY(say, causal || (a.K & 1) == 1, "dwconv: kernel size %d must be odd (non-causal)", a.K);
  M3_REQUIRE_SAY(say, !causal || a.K >= 2, "dwconv (causal): the frames left of frame 0 must be supplied (left_fill / cache)");
  M3_REQUIRE_SAY(say, !a.glu_sig || a.glu_ldz, "dwconv: sigmoided gate columns belong to the GLU-on-load form");
  return 0;
}
static DwKernArgs dwconv_pack(const DwArgs& q) {
  DwKernArgs k;
  k.z = q.z; k.w_kc = q.w_kc; k.bias = q.bias; k.gamma = q.gamma; k.beta = q.beta; k.eps = q.eps; k.T = q.T; k.D = q.D; k.K = q.K;
  k.out = q.out; k.out_bf16 = q.out_bf16; k.pad_of = q.pad_of; k.row0 = q.row0; k.row_len = q.row_len; k.n_rows = q.B * q.T;
  k.ldz = q.glu_ldz;
  k.cs.causal = dwconv_causal(q);
  k.cs.left = q.causal_left_fill;
  if (q.streaming) {   // the ping-pong cache [2][B][K-1][D], chunk counter(s) and valid frames on the device
    k.cs.left = q.cache_pair; k.cs.left_b_stride = (long)(q.K - 1) * q.D; k.cs.left_t_stride = q.D;
    k.cs.step = q.step; k.cs.half = (long)q.B * (q.K - 1) * q.D; k.cs.chunk_len = q.chunk_len;
    k.cs.max_chunks = q.slot_max_chunks > 0 ? q.slot_max_chunks : 0;
  }
  k.slots = q.streaming && q.slot_max_chunks >= 0;
  k.glu_in = q.glu_ldz ? (q.glu_sig ? 2 : 1) : 0;
  k.threads = (int)align_up(q.D / 4, 64);
  k.grid = k.n_rows + (q.streaming ? q.B * (q.K - 1) : 0);     // streaming: + the work-groups that write the new cache
  return k;
}
// The instantiation of a packed problem, named once for the single and the dual kernel: f(KT, CAUSAL, SLOTS, GLU_IN as constants)
template <int KT_, bool CAUSAL_, bool SLOTS_, int GLU_IN_>
struct DwForm { static constexpr int KT = KT_, GLU_IN = GLU_IN_; static constexpr bool CAUSAL = CAUSAL_, SLOTS = SLOTS_; };
template <class F>
static void dwconv_with_form(const DwKernArgs& k, F f) {
  if (k.glu_in == 2) f(DwForm<15, false, false, 2>{});
  else if (k.glu_in) f(DwForm<15, false, false, 1>{});
  else if (k.slots) { if (k.K <= 15) f(DwForm<15, true, true, 0>{}); else f(DwForm<8, true, true, 0>{}); }
  else if (k.K <= 15) { if (k.cs.causal) f(DwForm<15, true, false, 0>{}); else f(DwForm<15, false, false, 0>{}); }
  else { if (k.cs.causal) f(DwForm<8, true, false, 0>{}); else f(DwForm<8, false, false, 0>{}); }
}

int launch_dwconv_ln_silu(const DwArgs& a, hipStream_t stream) {
  if (int rc = check_dwconv(a)) return rc;
  const DwKernArgs k = dwconv_pack(a);
  if (k.n_rows == 0) return 0;
  dwconv_with_form(k, [&](auto f) {
    using F = decltype(f);
    hipLaunchKernelGGL((dwconv_ln_silu_kernel<F::KT, F::CAUSAL, F::SLOTS, F::GLU_IN>), dim3(k.grid), dim3(k.threads), 0, stream, k);
  });
  M3_LAUNCH_CHECK();
  return 0;
}
// two independent conv modules of the same shape class (channels, taps, causal or not, GLU on load or not) in ONE launch
bool dwconv_dual_fusable(const DwArgs& a, const DwArgs& b) {
  return check_dwconv(a, false) == 0 && check_dwconv(b, false) == 0 && !a.streaming && !b.streaming && a.D == b.D && a.K == b.K &&
         dwconv_causal(a) == dwconv_causal(b) && (a.glu_ldz != 0) == (b.glu_ldz != 0) && (a.glu_sig != 0) == (b.glu_sig != 0) &&
         a.B * a.T > 0 && b.B * b.T > 0;
}
int launch_dwconv_ln_silu_dual(const DwArgs& a, const DwArgs& b, hipStream_t stream) {
  M3_REQUIRE(dwconv_dual_fusable(a, b), "dwconv dual: the two problems do not share an instantiation");
  const DwKernArgs ka = dwconv_pack(a), kb = dwconv_pack(b);
  dwconv_with_form(ka, [&](auto f) {
    using F = decltype(f);
    hipLaunchKernelGGL((dwconv_ln_silu_dual_kernel<F::KT, F::CAUSAL, F::GLU_IN>), dim3(ka.grid + kb.grid), dim3(ka.threads), 0, stream, ka, kb);
  });
  M3_LAUNCH_CHECK();
  return 0;
}

// feat [B][T][idim] -> out [B][T1][F1][C] (channel-last), w9c [in_ch * 9][C] (repacked from (C,in_ch,3,3)), ReLU.
// Optional global CMVN folded into the read: x <- (x - mean[f]) * istd[f]   (the reference's unfinished CmvnPlugin,
// incomplete_plugin/cmvn_plugin/cmvn_plugin.cu:17-43; builder.sh:9 passes --cmvn_file but builder.py ignores it).
// One work-group per output row (b, t1): thread = 4 channels.  The thread's 9 x 4 weights and bias stay in registers,
// the three input rows (CMVN applied on the way) sit in LDS and are read as broadcasts, and the work-group walks the F1
// output columns writing C contiguous channels each -- no per-element index arithmetic, no weight reloads, 1-2 KB stores.
// (the body as a device function of the work-group's output row and column chunk: conv1_relu_dual_kernel runs the embed and the
//  main subsampler's first conv, which read the same features, in one launch)
// IN_CH > 1 (conv_subsample_in_ch of the reference, layer/subsampling.py:23-36): the idim columns of a frame are IN_CH blocks of
// Fc = idim / IN_CH bins (static | delta | delta-delta), read as the input channels of Conv2d(IN_CH, C, 3, 2): F1 counts on Fc,
// w9c is [IN_CH * 9][C] with row ch * 9 + kh * 3 + kw, the LDS tile stays [3][idim] and a tap sits at kh * idim + ch * Fc +
// 2 f1 + kw.  The thread keeps IN_CH * 9 f32x4 weights (27 at IN_CH = 3).  IN_CH = 1 is the one-channel code, tap for tap.
template <int IN_CH>
__device__ __forceinline__ void conv1_relu_body(const float* __restrict__ feat, const float* __restrict__ w9c,
                                                const float* __restrict__ bias, const float* __restrict__ cmvn_mean,
                                                const float* __restrict__ cmvn_istd, int T, int idim, int T1, int F1, int C,
                                                float* __restrict__ out, int relu, int out_bf16, const int32_t* __restrict__ feat_len,
                                                int32_t* __restrict__ lens_out, int B, const int row) {   // row = b * T1 + t1
  extern __shared__ float xs[];                       // [3][idim]
  // the engine's first launch also forms the valid lengths after the two stride-2 convs (both MaskConv2dSample applications,
  // subsampling.py:119-137) -- one launch less at the head of every forward
  if (feat_len != nullptr && row == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < B; i += blockDim.x) lens_out[i] = ((feat_len[i] - 3) / 2 + 1 - 3) / 2 + 1;
  const int b = row / T1, t1 = row - b * T1;
  const float* src = feat + ((size_t)b * T + 2 * t1) * idim;
  for (int i = threadIdx.x; i < 3 * idim; i += blockDim.x) {
    float xv = src[i];
    if (cmvn_mean != nullptr) {
      const int f = i % idim;
      xv = (xv - cmvn_mean[f]) * cmvn_istd[f];
    }
    xs[i] = xv;
  }
  const int c = threadIdx.x * 4;
  const bool live = c < C;
  f32x4 w[9 * IN_CH], bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (live) {
    bv = ldg4(bias + c);
#pragma unroll
    for (int k = 0; k < 9 * IN_CH; ++k) w[k] = ldg4(w9c + (size_t)k * C + c);
  }
  __syncthreads();
  if (!live) return;
  const size_t obase = (size_t)row * F1 * C + c;
  // short inputs: the F1 columns of a row are split over blockIdx.y so that a single utterance still fills the chip
  const int fchunk = (F1 + gridDim.y - 1) / gridDim.y;
  const int f_lo = blockIdx.y * fchunk, f_hi = min(F1, f_lo + fchunk);
  const int Fc = idim / IN_CH;
  for (int f1 = f_lo; f1 < f_hi; ++f1) {
    f32x4 acc = bv;
#pragma unroll
    for (int ch = 0; ch < IN_CH; ++ch)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const float xv = xs[kh * idim + ch * Fc + 2 * f1 + kw];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(xv, w[ch * 9 + kh * 3 + kw][j], acc[j]);
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = relu ? fmaxf(acc[j], 0.f) : acc[j];
    if (out_bf16) {
      bf16x4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = (bf16_t)acc[j];
      *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(out) + obase + (size_t)f1 * C) = h;
    } else {
      stg4(out + obase + (size_t)f1 * C, acc);
    }
  }
}

// One record per problem, filled by conv1_pack: the single kernel takes one, the dual kernel two.  T1, F1, the row count, the
// column split (short inputs: see conv1_relu_body) and the work-group size are derived there, once.
struct Conv1KernArgs {
  const float *feat, *w9c, *bias, *cmvn_mean, *cmvn_istd; int T, idim, T1, F1, C; float* out; int relu, out_bf16;
  const int32_t* feat_len; int32_t* lens_out; int B;
  int rows, fsplit, threads;   // the launch: B * T1 output rows, grid.y, block
};
#define M3_CONV1_SPREAD(a) a.feat, a.w9c, a.bias, a.cmvn_mean, a.cmvn_istd, a.T, a.idim, a.T1, a.F1, a.C, a.out, a.relu, a.out_bf16, a.feat_len, a.lens_out, a.B
template <int IN_CH>
__global__ __launch_bounds__(256) void conv1_relu_kernel(const Conv1KernArgs a) { conv1_relu_body<IN_CH>(M3_CONV1_SPREAD(a), (int)blockIdx.x); }
// both problems: the same input shape (B, T, idim) and the same in_ch, so the same T1, F1 and column split; the second
// problem's rows start at n0, a multiple of 8
template <int IN_CH>
__global__ __launch_bounds__(256) void conv1_relu_dual_kernel(const Conv1KernArgs a, const Conv1KernArgs b, int n0) {
  const int id = (int)blockIdx.x;
  if (id < n0) {
    if (id < a.rows) conv1_relu_body<IN_CH>(M3_CONV1_SPREAD(a), id);
  } else {
    conv1_relu_body<IN_CH>(M3_CONV1_SPREAD(b), id - n0);
  }
}
#undef M3_CONV1_SPREAD

static int check_conv1(const Conv1Args& a, bool say = true) {
  M3_REQUIRE_SAY(say, a.in_ch >= 1 && a.in_ch <= 3, "subsampling: in_ch=%d outside [1, 3]", a.in_ch);
  M3_REQUIRE_SAY(say, a.idim % a.in_ch == 0, "subsampling: idim=%d is no multiple of in_ch=%d", a.idim, a.in_ch);
  M3_REQUIRE_SAY(say, a.T >= 3 && a.idim / a.in_ch >= 3, "subsampling: input (T=%d, idim=%d / in_ch=%d) shorter than the 3x3 kernel", a.T, a.idim,
                 a.in_ch);
  M3_REQUIRE_SAY(say, (a.C & 3) == 0 && a.C > 0 && a.C <= 1024, "subsampling: channels=%d must be a multiple of 4 (<= 1024)", a.C);
  return 0;
}
static Conv1KernArgs conv1_pack(const Conv1Args& q) {
  Conv1KernArgs k;
  k.feat = q.feat; k.w9c = q.w9c; k.bias = q.bias; k.cmvn_mean = q.cmvn_mean; k.cmvn_istd = q.cmvn_istd; k.T = q.T; k.idim = q.idim;
  k.T1 = (q.T - 3) / 2 + 1; k.F1 = (q.idim / q.in_ch - 3) / 2 + 1; k.C = q.C; k.out = q.out; k.relu = q.relu; k.out_bf16 = q.out_bf16;
  k.feat_len = q.feat_len; k.lens_out = q.lens_out; k.B = q.B;
  k.rows = q.B * k.T1;
  k.fsplit = k.rows >= 2048 ? 1 : (k.rows >= 512 ? 2 : 5);
  k.threads = (int)align_up(q.C / 4, 64);
  return k;
}

int launch_conv1_relu(const Conv1Args& a, hipStream_t stream) {
  if (int rc = check_conv1(a)) return rc;
  const Conv1KernArgs k = conv1_pack(a);
  if (k.rows == 0) return 0;
  const dim3 grid(k.rows, k.fsplit), block(k.threads);
  const size_t lds = 3 * a.idim * sizeof(float);
  if (a.in_ch == 1) hipLaunchKernelGGL(conv1_relu_kernel<1>, grid, block, lds, stream, k);
  else if (a.in_ch == 2) hipLaunchKernelGGL(conv1_relu_kernel<2>, grid, block, lds, stream, k);
  else hipLaunchKernelGGL(conv1_relu_kernel<3>, grid, block, lds, stream, k);
  M3_LAUNCH_CHECK();
  return 0;
}
bool conv1_dual_fusable(const Conv1Args& a, const Conv1Args& b) {
  return check_conv1(a, false) == 0 && check_conv1(b, false) == 0 && a.B == b.B && a.T == b.T && a.idim == b.idim &&
         a.in_ch == b.in_ch && a.B * ((a.T - 3) / 2 + 1) > 0 && a.out != b.out;
}
int launch_conv1_relu_dual(const Conv1Args& a, const Conv1Args& b, hipStream_t stream) {
  M3_REQUIRE(conv1_dual_fusable(a, b), "subsampling conv1 dual: the two problems do not share an input shape and in_ch");
  const Conv1KernArgs ka = conv1_pack(a), kb = conv1_pack(b);
  const int n0 = (int)align_up((size_t)ka.rows, 8);
  const dim3 grid(n0 + kb.rows, ka.fsplit), block(ka.threads > kb.threads ? ka.threads : kb.threads);
  const size_t lds = 3 * a.idim * sizeof(float);
  if (a.in_ch == 1) hipLaunchKernelGGL(conv1_relu_dual_kernel<1>, grid, block, lds, stream, ka, kb, n0);
  else if (a.in_ch == 2) hipLaunchKernelGGL(conv1_relu_dual_kernel<2>, grid, block, lds, stream, ka, kb, n0);
  else hipLaunchKernelGGL(conv1_relu_dual_kernel<3>, grid, block, lds, stream, ka, kb, n0);
  M3_LAUNCH_CHECK();
  return 0;
}

// y (B,C,To) = depthwise conv of x (B,C,T), To = T + 2 pad - K + 1 (nn.Conv1d: pad = (K-1)/2 keeps the length, the
// causal module pads its input itself and convolves with pad = 0, convolution.py:43-49)
__global__ void depthwise_conv1d_nct_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                            const float* __restrict__ bias, int C, int T, int To, int K, int pad,
                                            float* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % To);
    const size_t bc = i / To;
    const int c = (int)(bc % C);
    const float* xr = x + bc * T;
    float acc = bias ? bias[c] : 0.f;
    for (int k = 0; k < K; ++k) {
      const int tt = t + k - pad;
      if (tt >= 0 && tt < T) acc = fmaf(xr[tt], w[(size_t)c * K + k], acc);
    }
    y[i] = acc;
  }
}

int launch_depthwise_conv1d_nct(const float* x, const float* w, const float* bias, int B, int C, int T, int K,
                                int pad, float* y, hipStream_t stream) {
  const int To = T + 2 * pad - K + 1;
  M3_REQUIRE(pad >= 0 && To > 0, "depthwise_conv1d: T=%d K=%d pad=%d leaves no output", T, K, pad);
  const size_t n = (size_t)B * C * To;
  if (n == 0) return 0;
  hipLaunchKernelGGL(depthwise_conv1d_nct_kernel, dim3(grid1d(n, 4096)), dim3(256), 0,
                     stream, x, w, bias, C, T, To, K, pad, y, n);
  M3_LAUNCH_CHECK();
  return 0;
}

// zero padding of the last two dims: x (outer, H, W) -> y (outer, H + pre_h + post_h, W + pre_w + post_w)
// (TensorRT IPaddingLayer, network.add_padding in the causal conv module, convolution.py:118-123)
__global__ void pad2d_kernel(const float* __restrict__ x, int H, int W, int pre_h, int pre_w, int Ho, int Wo,
                             float* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int wo = (int)(i % Wo), ho = (int)((i / Wo) % Ho);
    const size_t o = i / ((size_t)Wo * Ho);
    const int h = ho - pre_h, w_ = wo - pre_w;
    y[i] = (h >= 0 && h < H && w_ >= 0 && w_ < W) ? x[(o * H + h) * W + w_] : 0.f;
  }
}
int launch_pad2d(const float* x, size_t outer, int H, int W, int pre_h, int post_h, int pre_w, int post_w, float* y, hipStream_t stream) {
  M3_REQUIRE(pre_h >= 0 && post_h >= 0 && pre_w >= 0 && post_w >= 0, "pad2d: negative padding (cropping) is not implemented");
  const int Ho = H + pre_h + post_h, Wo = W + pre_w + post_w;
  const size_t n = outer * Ho * Wo;
  if (n == 0) return 0;
  hipLaunchKernelGGL(pad2d_kernel, dim3(grid1d(n, 4096)), dim3(256), 0, stream, x, H, W, pre_h, pre_w, Ho, Wo, y, n);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
