// Split-K LDS-tiled fp32 GEMM for the two deep-K layers of the subsampling front end at short inputs.
//
//   conv2  (Conv2d 3x3 stride 2, C->C, as implicit GEMM):  M = B*T2*F2 = 450,  N = 512, K = 9*C = 4608
//   out.0  (Linear(C*F2 -> D)):                             M = B*T' = 50,      N = 512, K = 9728
// (reference: TensorRT convolution / matmul layers built by torch_network_helper.py:227-251,573-605 from
// layer/subsampling.py:103-145).  The K-split kernel of gemm.hip gives every 16-column workgroup its own copy of the
// im2col rows: at B=1 conv2 moved ~820 MB through L2 for 2.1 GFLOP and took 58 us, 5 % of a forward.  Here the output is
// cut into 64 x 64 tiles and K into `splits` ranges; one workgroup = (tile, K range) runs the pipeline of
// moe_expert_tiled_f32.hip (coalesced 16-B staging loads one k-step ahead, 2-stage LDS ring, 2x2 waves of 32x32,
// v_mfma_f32_16x16x4_f32) and writes its raw partial tile; splitk_reduce_kernel sums the partials in a fixed order
// and applies bias / ReLU / scale (deterministic, no atomics).  Partials live in the engine workspace.
#include "common.h"
#include "kernels.h"

namespace m3 {

namespace {
constexpr int SBM = 64, SBN = 64, SBK = 64;
constexpr int S_LD = SBK + 4;                        // floats per LDS row (272 B: conflict-free 16-B reads)
constexpr int SC_LD = SBN + 4;
constexpr int kSplitLdsBytes = 2 * (SBM + SBN) * S_LD * 4;   // 69,632 B (the 17 KB epilogue image reuses it)
}  // namespace

// The kernel body as a device function of (parameter block, output tile, K range): gemm_f32_splitk_kernel runs one problem,
// gemm_f32_splitk_dual_kernel two INDEPENDENT problems in one launch -- the embed and the main subsampler read the same features
// through different weights (engine.hip "horizontal fusion").  Each problem keeps its own split count and partial tiles.
template <bool CONV>
__device__ __forceinline__ void gemm_f32_splitk_body(const GemmParams& p, float* __restrict__ part, const int ksteps_per_split,
                                                     const int tile_id, const int split) {
  constexpr int MT = SBM / 32, NT = SBN / 32;
  constexpr int CA = SBK / 4, RA = 256 / CA, JA = SBM / RA, JB = SBN / RA;
  extern __shared__ __attribute__((aligned(16))) unsigned char splitk_lds[];
  float* As = reinterpret_cast<float*>(splitk_lds);
  float* Bs = As + 2 * SBM * S_LD;
  float* Cs = reinterpret_cast<float*>(splitk_lds);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int n_tile = tile_id % p.n_tiles, m_tile = tile_id / p.n_tiles;
  const int m0 = m_tile * SBM, n0 = n_tile * SBN;
  const int nsteps_total = p.K / SBK;
  const int s_lo = split * ksteps_per_split, s_hi = min(s_lo + ksteps_per_split, nsteps_total);

  const int ac = tid % CA, ar0 = tid / CA;
  const float* aptr[JA];
#pragma unroll
  for (int j = 0; j < JA; ++j) {
    const int m = min(m0 + ar0 + RA * j, p.M - 1);
    if (CONV) {
      const int f2 = m % p.conv_F2;
      const int t2 = (m / p.conv_F2) % p.conv_T2;
      const int b = m / (p.conv_F2 * p.conv_T2);
      aptr[j] = p.A + ((size_t)(b * p.conv_T1 + 2 * t2) * p.conv_F1 + 2 * f2) * p.conv_C + 4 * ac;
    } else {
      aptr[j] = p.A + (size_t)m * p.lda + 4 * ac;
    }
  }
  const float* bptr[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) bptr[j] = p.W + (size_t)min(n0 + ar0 + RA * j, p.N - 1) * p.K + 4 * ac;
  auto a_offset = [&](int k) -> int {
    if (CONV) {
      const int seg = k / p.conv_C, c = k - seg * p.conv_C;
      const int kh = seg / 3, kw = seg - kh * 3;
      return (kh * p.conv_F1 + kw) * p.conv_C + c;
    }
    return k;
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 areg[JA], breg[JB];
  auto load_tiles = [&](int s) {
    const int ko = a_offset(s * SBK);
#pragma unroll
    for (int j = 0; j < JA; ++j) areg[j] = ldg4(aptr[j] + ko);
#pragma unroll
    for (int j = 0; j < JB; ++j) breg[j] = ldg4_w(bptr[j] + s * SBK);
  };
  auto store_tiles = [&](int buf) {
    float* a_dst = As + buf * (SBM * S_LD) + ar0 * S_LD + 4 * ac;
    float* b_dst = Bs + buf * (SBN * S_LD) + ar0 * S_LD + 4 * ac;
#pragma unroll
    for (int j = 0; j < JA; ++j) *reinterpret_cast<f32x4*>(a_dst + RA * j * S_LD) = areg[j];
#pragma unroll
    for (int j = 0; j < JB; ++j) *reinterpret_cast<f32x4*>(b_dst + RA * j * S_LD) = breg[j];
  };

  load_tiles(s_lo);
  store_tiles(0);
  __syncthreads();
  for (int s = s_lo; s < s_hi; ++s) {
    const int i = s - s_lo;
    load_tiles(min(s + 1, s_hi - 1));                // clamped, unconditional (see gemm_bf16_tiled.hip)
    __builtin_amdgcn_sched_barrier(0);
    const float* a_lds = As + (i & 1) * (SBM * S_LD) + ((SBM / 2) * wm + col) * S_LD + 4 * kq;
    const float* b_lds = Bs + (i & 1) * (SBN * S_LD) + ((SBN / 2) * wn + col) * S_LD + 4 * kq;
#pragma unroll
    for (int ks = 0; ks < SBK / 16; ++ks) {
      f32x4 b[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = *reinterpret_cast<const f32x4*>(b_lds + 16 * nt * S_LD + 16 * ks);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(a_lds + 16 * mt * S_LD + 16 * ks);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[mt][nt] = mfma16(a[j], b[nt][j], acc[mt][nt]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    store_tiles((i + 1) & 1);
    __syncthreads();
  }

#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Cs[((SBM / 2) * wm + 16 * mt + 4 * kq + r) * SC_LD + (SBN / 2) * wn + 16 * nt + col] = acc[mt][nt][r];
  __syncthreads();
  // raw partial tile -> part[split][m][n] (row-wise, float4 per lane)
  const int c4 = 4 * (lane & 15), n = n0 + c4;
  for (int it = 0; it < SBM / 16; ++it) {
    const int row = (4 * it + wave) * 4 + (lane >> 4);
    const int m = m0 + row;
    if (m < p.M && n < p.N) stg4(part + ((size_t)split * p.M + m) * p.N + n, *reinterpret_cast<const f32x4*>(Cs + row * SC_LD + c4));
  }
}

template <bool CONV>
__global__ __launch_bounds__(256, 2) void gemm_f32_splitk_kernel(const GemmParams p, float* __restrict__ part,
                                                                 int ksteps_per_split) {
  gemm_f32_splitk_body<CONV>(p, part, ksteps_per_split, (int)blockIdx.x, (int)blockIdx.y);
}
// work-groups [0, live0) are problem 0's (tile fastest, then K range, the order of the two-dimensional grid), [n0, ...) problem
// 1's; n0 = live0 rounded up to a multiple of 8, the ids between do nothing
template <bool CONV>
__global__ __launch_bounds__(256, 2) void gemm_f32_splitk_dual_kernel(const GemmParams p0, float* __restrict__ part0, int per0, int live0,
                                                                      const GemmParams p1, float* __restrict__ part1, int per1, int n0) {
  const int id = (int)blockIdx.x;
  if (id < n0) {
    const int tiles = p0.m_tiles * p0.n_tiles;
    if (id < live0) gemm_f32_splitk_body<CONV>(p0, part0, per0, id % tiles, id / tiles);
  } else {
    const int tiles = p1.m_tiles * p1.n_tiles;
    gemm_f32_splitk_body<CONV>(p1, part1, per1, (id - n0) % tiles, (id - n0) / tiles);
  }
}

// y[m][n] = alpha * act(bias[n] + sum_s part[s][m][n]), fixed summation order
// (as a device function of the work-group's place among the `nblocks` of its problem: splitk_reduce_dual_kernel)
__device__ __forceinline__ void splitk_reduce_body(const float* __restrict__ part, int splits, int M, int N,
                                                   const float* __restrict__ bias, int act, float alpha,
                                                   float* __restrict__ y, int ldy, const int bid, const int nblocks) {
  const size_t quads = (size_t)M * (N / 4);
  for (size_t q = (size_t)bid * 256 + threadIdx.x; q < quads; q += (size_t)nblocks * 256) {
    const int m = (int)(q / (N / 4)), n = 4 * (int)(q % (N / 4));
    f32x4 v = bias ? ldg4(bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < splits; s0 += 4) {          // 4 partials in flight
      f32x4 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        t[j] = (s0 + j < splits) ? ldg4(part + ((size_t)(s0 + j) * M + m) * N + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) v += t[j];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = v[e];
      if (act == ACT_RELU) t = fmaxf(t, 0.f);
      if (act == ACT_SILU) t = silu(t);
      v[e] = t * alpha;
    }
    stg4(y + (size_t)m * ldy + n, v);
  }
}

__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splits, int M, int N,
                                                            const float* __restrict__ bias, int act, float alpha,
                                                            float* __restrict__ y, int ldy) {
  splitk_reduce_body(part, splits, M, N, bias, act, alpha, y, ldy, (int)blockIdx.x, (int)gridDim.x);
}
struct SplitkReduceArgs { const float* part; int splits, M, N; const float* bias; int act; float alpha; float* y; int ldy; int nblocks; };
__global__ __launch_bounds__(256) void splitk_reduce_dual_kernel(const SplitkReduceArgs a, const SplitkReduceArgs b) {
  if ((int)blockIdx.x < a.nblocks)
    splitk_reduce_body(a.part, a.splits, a.M, a.N, a.bias, a.act, a.alpha, a.y, a.ldy, (int)blockIdx.x, a.nblocks);
  else
    splitk_reduce_body(b.part, b.splits, b.M, b.N, b.bias, b.act, b.alpha, b.y, b.ldy, (int)blockIdx.x - a.nblocks, b.nblocks);
}

int init_gemm_f32_splitk_kernels() {
  static PerDeviceOnce once;
  if (once.done()) return 0;
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_f32_splitk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kSplitLdsBytes));
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_f32_splitk_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kSplitLdsBytes));
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_f32_splitk_dual_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kSplitLdsBytes));
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_f32_splitk_dual_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kSplitLdsBytes));
  once.mark();
  return 0;
}

int launch_gemm_f32_splitk(const GemmPlan& plan, const GemmParams& pin, float* ws, hipStream_t stream) {
  GemmParams p = pin;
  if (int rc = init_gemm_f32_splitk_kernels()) return rc;
  const int splits = plan.splits;
  p.m_tiles = plan.m_tiles; p.n_tiles = plan.n_tiles;
  const int per = cdiv(p.K / SBK, splits);
  dim3 grid(p.m_tiles * p.n_tiles, splits);
  if (plan.conv)
    hipLaunchKernelGGL((gemm_f32_splitk_kernel<true>), grid, dim3(256), kSplitLdsBytes, stream, p, ws, per);
  else
    hipLaunchKernelGGL((gemm_f32_splitk_kernel<false>), grid, dim3(256), kSplitLdsBytes, stream, p, ws, per);
  const size_t quads = (size_t)p.M * (p.N / 4);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid1d(quads, 1024)), dim3(256), 0, stream, ws, splits, p.M, p.N, p.bias, p.act,
                     p.alpha, p.Y, p.ldy);
  M3_LAUNCH_CHECK();
  return 0;
}

// two independent split-K problems (both implicit convs or both plain) in ONE GEMM launch and ONE reduce launch: each keeps its
// split count, its partial tiles and its reduce order, so each result is what launch_gemm_f32_splitk gives, bit for bit.
// `which`: 1 = the GEMM launch, 2 = the reduce launch, 3 = both (the engine lists them as two stages)
bool gemm_splitk_dual_fusable(const GemmLaunch& ga, const GemmLaunch& gb) {
  const GemmPlan &a = ga.plan, &b = gb.plan;
  return a.launches == 2 && b.launches == 2 && a.kernel == GemmKernel::SplitKF32 && b.kernel == GemmKernel::SplitKF32 && a.conv == b.conv &&
         ga.ws != nullptr && gb.ws != nullptr && ga.ws != gb.ws;
}
int launch_gemm_f32_splitk_dual(const GemmLaunch& a, const GemmLaunch& b, hipStream_t stream, int which) {
  M3_REQUIRE(a.ws != nullptr && b.ws != nullptr && a.ws != b.ws, "gemm split-K dual: each problem needs its own workspace");
  M3_REQUIRE(gemm_splitk_dual_fusable(a, b), "gemm split-K dual: the two problems do not share an instantiation");
  if (int rc = init_gemm_f32_splitk_kernels()) return rc;
  GemmParams q[2] = {a.p, b.p};
  const GemmPlan* const plans[2] = {&a.plan, &b.plan};
  int per[2], live[2];
  SplitkReduceArgs r[2];
  float* const ws[2] = {a.ws, b.ws};
  for (int i = 0; i < 2; ++i) {
    q[i].m_tiles = plans[i]->m_tiles; q[i].n_tiles = plans[i]->n_tiles;
    per[i] = cdiv(q[i].K / SBK, plans[i]->splits);
    live[i] = q[i].m_tiles * q[i].n_tiles * plans[i]->splits;
    r[i] = SplitkReduceArgs{ws[i], plans[i]->splits, q[i].M, q[i].N, q[i].bias, q[i].act, q[i].alpha, q[i].Y, q[i].ldy,
                            (int)grid1d((size_t)q[i].M * (q[i].N / 4), 1024)};
  }
  const int n0 = (int)align_up((size_t)live[0], 8);
  const dim3 grid(n0 + live[1]);
  if ((which & 1) && a.plan.conv)
    hipLaunchKernelGGL((gemm_f32_splitk_dual_kernel<true>), grid, dim3(256), kSplitLdsBytes, stream, q[0], ws[0], per[0], live[0], q[1], ws[1], per[1], n0);
  else if (which & 1)
    hipLaunchKernelGGL((gemm_f32_splitk_dual_kernel<false>), grid, dim3(256), kSplitLdsBytes, stream, q[0], ws[0], per[0], live[0], q[1], ws[1], per[1], n0);
  if (which & 2) hipLaunchKernelGGL(splitk_reduce_dual_kernel, dim3(r[0].nblocks + r[1].nblocks), dim3(256), 0, stream, r[0], r[1]);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
