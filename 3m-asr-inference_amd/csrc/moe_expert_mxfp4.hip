// Grouped expert FFN with OCP MXFP4 expert weights: W4A16.
//
// The fourth storage mode of the expert weights (fp32 / bf16 / fp8 / mxfp4).  At one utterance the operator is a weight
// stream (moe_expert_fp8.hip): 0.53 MB per touched expert at D = 512, F = 1024 instead of 1.05 (fp8).  The format is the one
// m3asr/plan.py quantize_mxfp4 defines: e2m1 elements (sign in bit 3 of a code, magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}), two
// codes per byte with the even-k element in the low nibble, and one e8m0 scale byte per 32 consecutive k.  Weights are decoded
// to bf16 in registers by v_cvt_scalef32_pk_bf16_fp4 (two nibbles and the block's scale -> two bf16, the byte of the dword
// picked by op_sel) on their way to v_mfma_f32_16x16x32_bf16.  Every e2m1 value times a power of two is exact in bf16, rows
// and H stay bf16 in LDS and accumulation is fp32, so the arithmetic is that of the bf16 kernel on the decoded weights: the
// only new error is the weight quantisation.  The scale varies along k, so it is applied at decode; nothing scales the
// accumulator here.
//
// Same decomposition as moe_expert_fp8.hip (work item = (expert, 64-wide hidden slice), rows and H in LDS as bf16, slab
// partials, shared combine, two register groups in flight).  Lane maps:
//   phase 1  a step is 128 deep.  Lane (col, kq) loads 16 bytes of W1 row n = f0 + 16 wave + col: k = 128 s + 32 kq + [0, 32),
//            exactly one MX block, and its one scale byte.  Dword j of the load holds k = 128 s + 32 kq + 8 j + [0, 8) and feeds
//            MFMA j of the step; the A fragment is read from LDS at the same k (any assignment of k to MFMA slots is valid when
//            both operands agree).  A group is 4 steps (16 dwords).
//   phase 2  the slice's 64 k are two blocks.  Lane (col, kq) loads 8 bytes of W2 row d = 16 sub + col: k = 16 kq + [0, 16),
//            with the scale of block kq >> 1; dword 0 / 1 pair with hfrag[.][0] / [1] as in the fp8 kernel.  A group is 8 output
//            tiles (16 dwords: the same registers as a phase-1 group).
// A-fragment reads: 16-byte ds_read at row (col) stride (D + 8) bf16 = 4 dwords mod 64 banks, so the 16 lanes of one kq cover
// the 64 banks once whatever k offset kq adds (the pattern of the bf16 and fp8 kernels, with another constant per kq).
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace m3 {

template <int MT>
__global__ __launch_bounds__(64 * (kExpertSliceW16 / 16)) void expert_ffn_w4_kernel(
    const float* __restrict__ x, int ldx, const int32_t* __restrict__ pos, const int32_t* __restrict__ acc_hist, int S,
    int D, int F, const uint8_t* __restrict__ w1, const uint8_t* __restrict__ s1, const float* __restrict__ b1,
    const uint8_t* __restrict__ w2, const uint8_t* __restrict__ s2, int w2_row_stride, int w2_slice_stride,
    int s2_row_stride, int s2_slice_stride, float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw4[];
  const int e = blockIdx.y, slice = blockIdx.x;
  const int row_lo = acc_hist[e], row_hi = acc_hist[e + 1];
  if (row_hi <= row_lo) return;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int xs_ld = D + 8;
  constexpr int hs_ld = kExpertSliceW16 + 8;
  constexpr int NWV = kExpertSliceW16 / 16;
  static_assert(kExpertSliceW16 == 64, "laid out for 64-wide slices (two MX blocks)");
  bf16_t* xs = reinterpret_cast<bf16_t*>(lds_raw4);   // [16*MT][D+8]
  bf16_t* hs = xs + 16 * MT * xs_ld;                  // [16*MT][64+8]
  const int f0 = slice * kExpertSliceW16;
  const int kd1 = D >> 7;                             // 128-deep steps of phase 1
  const int n1 = f0 + 16 * wave + col;                // this lane's hidden unit

  // byte strides: two codes per byte, one scale byte per 32 k
  const uint8_t* w1row = w1 + ((size_t)e * F + n1) * (D >> 1) + 16 * kq;
  const uint8_t* s1row = s1 + ((size_t)e * F + n1) * (D >> 5) + kq;
  const float bias1 = b1[(size_t)e * F + n1];
  const int nsub = D >> 4;                            // 16-column output tiles of phase 2
  const int tpw = (nsub + NWV - 1) / NWV;             // tiles per wave
  const uint8_t* w2_slice = w2 + (size_t)e * D * (F >> 1) + (size_t)slice * w2_slice_stride + 8 * kq;
  const uint8_t* s2_slice = s2 + (size_t)e * D * (F >> 5) + (size_t)slice * s2_slice_stride + (kq >> 1);

  const int g1 = (kd1 + 3) >> 2, g2 = (tpw + 7) >> 3;
  const int total = g1 + g2;

  for (int r0 = row_lo + 16 * MT * blockIdx.z; r0 < row_hi; r0 += 16 * MT * gridDim.z) {
    const int nrows = min(16 * MT, row_hi - r0);
    float* slab_base = slab + ((size_t)slice * S + r0) * D;

    unsigned int wb[2][16];                           // 4 x 16 bytes (phase 1) or 8 x 8 bytes (phase 2)
    unsigned int sc[2][8];                            // the e8m0 code of each load's block
    auto load_group = [&](int g, int buf) {
      if (g < g1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int s = min(4 * g + i, kd1 - 1);          // clamped, not branched
          const u32x4 v = ldg16b_w(w1row + (s << 6));
#pragma unroll
          for (int j = 0; j < 4; ++j) wb[buf][4 * i + j] = v[j];
          sc[buf][i] = s1row[s << 2];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int sub = min(wave + NWV * (8 * (g - g1) + j), nsub - 1);
          const u32x2 v = ldg8b_w(w2_slice + (size_t)(16 * sub + col) * w2_row_stride);
          wb[buf][2 * j] = v[0];
          wb[buf][2 * j + 1] = v[1];
          sc[buf][j] = s2_slice[(size_t)(16 * sub + col) * s2_row_stride];
        }
      }
    };
    load_group(0, 0);

    // ---- gather token rows into LDS, rounded to bf16 (fused local_scatter) ----
    __syncthreads();
    for (int i = wave; i < 16 * MT; i += NWV) {
      bf16_t* dst = xs + i * xs_ld;
      if (i < nrows) {
        const float* src = x + (size_t)pos[r0 + i] * ldx;
        for (int c = lane * 8; c < D; c += 512)
          *reinterpret_cast<bf16x8*>(dst + c) = cvt8(ldg4(src + c), ldg4(src + c + 4));
      } else {
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.f;
        for (int c = lane * 8; c < D; c += 512) *reinterpret_cast<bf16x8*>(dst + c) = z;
      }
    }
    __syncthreads();

    f32x4 acc1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 hfrag[MT][2];

    auto transition = [&]() {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          hs[(16 * mt + 4 * kq + r) * hs_ld + 16 * wave + col] = (bf16_t)silu(acc1[mt][r] + bias1);
      __syncthreads();
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int half = 0; half < 2; ++half)
          hfrag[mt][half] = *reinterpret_cast<const bf16x8*>(hs + (16 * mt + col) * hs_ld + 16 * kq + 8 * half);
    };
    auto compute = [&](int g, int buf) {
      if (g < g1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int s = 4 * g + i;
          if (s < kd1) {
            const float scale = e8m0_to_f32(sc[buf][i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bf16x8 b = mxfp4x8_to_bf16(wb[buf][4 * i + j], scale);
#pragma unroll
              for (int mt = 0; mt < MT; ++mt) {
                const bf16_t* ap = xs + (16 * mt + col) * xs_ld + (s << 7) + 32 * kq + 8 * j;
                acc1[mt] = mfma16h(*reinterpret_cast<const bf16x8*>(ap), b, acc1[mt]);
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int sub = wave + NWV * (8 * (g - g1) + j);
          if (sub < nsub) {
            const float scale = e8m0_to_f32(sc[buf][j]);
            const bf16x8 blo = mxfp4x8_to_bf16(wb[buf][2 * j], scale);
            const bf16x8 bhi = mxfp4x8_to_bf16(wb[buf][2 * j + 1], scale);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              f32x4 acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
              acc2 = mfma16h(hfrag[mt][0], blo, acc2);
              acc2 = mfma16h(hfrag[mt][1], bhi, acc2);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int i = 16 * mt + 4 * kq + r;
                if (i < nrows) slab_base[(size_t)i * D + 16 * sub + col] = acc2[r];
              }
            }
          }
        }
      }
    };

    for (int g0 = 0; g0 < total; g0 += 2) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int g = g0 + b;
        if (g < total) {
          if (g + 1 < total) load_group(g + 1, b ^ 1);
          if (g == g1) transition();
          compute(g, b);
        }
      }
    }
  }
}

int init_expert_ffn_w4_kernels() {
  static PerDeviceOnce once;
  if (once.done()) return 0;
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)expert_ffn_w4_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  once.mark();
  return 0;
}

// MXFP4 expert weights: w1 [E][F][D/2] codes + s1 [E][F][D/32] scale bytes; w2 [E][D][F/2] + s2 [E][D][F/32], or slice-major
// [E][F/64][D][32] + [E][F/64][D][2].  Result layout (F / 64 slabs) is that of the bf16 slab form; the tiled (long-batch) form
// lives in gemm_bf16_tiled.hip.
int launch_expert_ffn_w4_slab(const float* x, int ldx, const int32_t* pos, const int32_t* acc_hist, int S, int E, int D, int F,
                              const void* w1, const void* s1, const float* b1, const void* w2, const void* s2, int w2_sliced,
                              float* slab, hipStream_t stream) {
  M3_REQUIRE(S > 0 && E > 0, "expert_ffn_w4: empty problem S=%d E=%d", S, E);
  M3_REQUIRE((D & 127) == 0 && D <= 2048, "expert_ffn_w4: idim=%d must be a multiple of 128 (<=2048)", D);
  M3_REQUIRE(F % kExpertSliceW16 == 0, "expert_ffn_w4: hidden_units=%d must be a multiple of %d", F, kExpertSliceW16);
  M3_REQUIRE((ldx & 3) == 0 && ldx >= D, "expert_ffn_w4: ldx=%d must be a multiple of 4 and at least idim=%d", ldx, D);
  M3_REQUIRE(w1 && s1 && w2 && s2, "expert_ffn_w4: null weights or scales");
  const int mt = S <= 64 ? 1 : (S <= 512 ? 2 : 4);
  const size_t lds_bytes = (size_t)16 * mt * ((D + 8) + (kExpertSliceW16 + 8)) * sizeof(bf16_t);
  M3_REQUIRE(lds_bytes <= 160 * 1024, "expert_ffn_w4: LDS tile of %zu bytes does not fit", lds_bytes);
  int zt = cdiv(S, 16 * mt);
  dim3 grid(F / kExpertSliceW16, E, zt < 8 ? zt : 8);
  // bytes: a slice of a W2 row is 32 bytes of codes and 2 scale bytes
  const int w2_row_stride = w2_sliced ? kExpertSliceW16 / 2 : F / 2;
  const int w2_slice_stride = w2_sliced ? D * (kExpertSliceW16 / 2) : kExpertSliceW16 / 2;
  const int s2_row_stride = w2_sliced ? 2 : F / 32;
  const int s2_slice_stride = w2_sliced ? D * 2 : 2;
  if (int rc = init_expert_ffn_w4_kernels()) return rc;
#define M3_EXPERT_CASE(MT_)                                                                                           \
  hipLaunchKernelGGL((expert_ffn_w4_kernel<MT_>), grid, dim3(64 * (kExpertSliceW16 / 16)), lds_bytes, stream, x, ldx, pos, \
                     acc_hist, S, D, F, (const uint8_t*)w1, (const uint8_t*)s1, b1, (const uint8_t*)w2, (const uint8_t*)s2, \
                     w2_row_stride, w2_slice_stride, s2_row_stride, s2_slice_stride, slab)
  if (mt == 1) M3_EXPERT_CASE(1); else if (mt == 2) M3_EXPERT_CASE(2); else M3_EXPERT_CASE(4);
#undef M3_EXPERT_CASE
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
