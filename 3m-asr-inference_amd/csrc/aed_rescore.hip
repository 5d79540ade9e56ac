// Attention rescoring: the three kernels the AED decoder's second pass needs besides the dense GEMMs
// (m3_linear) -- decoder input rows from the device n-best, the multi-head attention core on packed hypothesis rows, and the
// per-hypothesis score with the per-utterance choice.  fp32 throughout, no atomics, every reduction in a fixed order, and a
// row's result does not depend on where the row lies in the batch.
#include <math.h>

#include "../../include/m3asr.h"
#include "common.h"

namespace m3 {

// ---------------------------------------------------------------------------------------------------------------- embed
// one work-group per hypothesis slot h = b * beam + i: rows [hyp_row0[h], hyp_row0[h + 1]) = sos, then the tokens
__global__ __launch_bounds__(256) void aed_embed_kernel(const int32_t* __restrict__ hyp_tokens, const int32_t* __restrict__ hyp_len,
                                                        const int32_t* __restrict__ n_hyps, const int32_t* __restrict__ hyp_row0,
                                                        int beam, int max_frames, const float* __restrict__ emb,
                                                        const float* __restrict__ pe, int pe_rows, int V, int D, int reverse,
                                                        int rows, float sqrt_d, float* __restrict__ x, int ldx,
                                                        int32_t* __restrict__ target) {
  const int h = blockIdx.x, b = h / beam, i = h - b * beam;
  if (i >= n_hyps[b]) return;                                      // dead slot (n_hyps < 0: a failed search)
  const int n = hyp_len[h], row0 = hyp_row0[h];
  if (n < 0 || n > max_frames || n + 1 > pe_rows || row0 < 0 || hyp_row0[h + 1] - row0 != n + 1 || row0 + n + 1 > rows) return;
  const int32_t* y = hyp_tokens + (size_t)h * max_frames;
  const int sos = V - 1, d4 = D >> 2;
  for (int r = 0; r <= n; ++r) {
    const int tok = r == 0 ? sos : (reverse ? y[n - r] : y[r - 1]);
    const bool ok = tok >= 0 && tok < V;
    float* xr = x + (size_t)(row0 + r) * ldx;
    for (int c = threadIdx.x; c < d4; c += blockDim.x) {
      f32x4 o;
      if (ok) {
        const f32x4 e = ldg4(emb + (size_t)tok * D + 4 * c), p = ldg4(pe + (size_t)r * D + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = e[j] * sqrt_d + p[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = NAN;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) xr[4 * c + j] = o[j];
    }
    if (threadIdx.x == 0) target[row0 + r] = r < n ? (reverse ? y[n - 1 - r] : y[r]) : sos;
  }
}

// ------------------------------------------------------------------------------------------------------------ attention
constexpr int AED_KT = 64;        // keys per LDS tile: one per lane of a wave
constexpr int AED_QW = 4;         // queries a wave carries through the key tiles
constexpr int AED_QT = 4 * AED_QW;  // queries per work-group (4 waves)

template <int DK>
constexpr size_t aed_attention_lds_bytes() {
  return sizeof(float) * ((size_t)AED_KT * (DK + 1) + (size_t)AED_KT * DK + (size_t)AED_QT * DK);
}

__device__ __forceinline__ float lane_bcast(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// grid (slot, head, query tile).  The work-group stages 64 keys and values of its head in LDS (K rows padded to DK + 1 floats:
// lane j reads row j), every wave takes 4 queries: lane j scores key j against them, the tile's maximum and sum go through
// the wave, and lane d accumulates output dimension d (and d + 64) with the probabilities broadcast from their lanes.
template <int DK>
__global__ __launch_bounds__(256) void aed_attention_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                            int ldk, const float* __restrict__ v, int ldv,
                                                            const int32_t* __restrict__ desc, int q_rows, int kv_rows,
                                                            float scale, float* __restrict__ out, int ldo) {
  constexpr int DPL = (DK + 63) / 64, KS = DK + 1, C4 = DK / 4;
  extern __shared__ float aed_lds[];
  float* Ks = aed_lds;
  float* Vs = Ks + AED_KT * KS;
  float* Qs = Vs + AED_KT * DK;
  const int32_t* d = desc + (size_t)blockIdx.x * 5;
  const int q_row0 = d[0], n_q = d[1], kv_row0 = d[2], kv_len = d[3], causal = d[4];
  const int head = blockIdx.y, q_lo = blockIdx.z * AED_QT;
  if (n_q <= 0 || q_lo >= n_q) return;
  if (kv_len <= 0 || q_row0 < 0 || n_q > q_rows - q_row0 || kv_row0 < 0 || kv_len > kv_rows - kv_row0) return;
  const int nq = min(AED_QT, n_q - q_lo);
  const int kv_end = causal ? min(kv_len, q_lo + nq) : kv_len;    // no query of this tile sees a key past its own position
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t col0 = (size_t)head * DK;

  for (int idx = tid; idx < AED_QT * C4; idx += 256) {
    const int r = idx / C4, c = idx - r * C4;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (r < nq) t = ldg4(q + (size_t)(q_row0 + q_lo + r) * ldq + col0 + 4 * c);
    stg4(Qs + r * DK + 4 * c, t);
  }

  float m[AED_QW], l[AED_QW], o[AED_QW][DPL];
#pragma unroll
  for (int t = 0; t < AED_QW; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int c = 0; c < DPL; ++c) o[t][c] = 0.f;
  }

  for (int t0 = 0; t0 < kv_end; t0 += AED_KT) {
    __syncthreads();                                               // the previous tile has been read (and Qs written)
    for (int idx = tid; idx < AED_KT * C4; idx += 256) {
      const int j = idx / C4, c = idx - j * C4;
      f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (t0 + j < kv_end) {
        kk = ldg4(k + (size_t)(kv_row0 + t0 + j) * ldk + col0 + 4 * c);
        vv = ldg4(v + (size_t)(kv_row0 + t0 + j) * ldv + col0 + 4 * c);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) Ks[j * KS + 4 * c + e] = kk[e];
      stg4(Vs + j * DK + 4 * c, vv);
    }
    __syncthreads();

    float s[AED_QW];
#pragma unroll
    for (int t = 0; t < AED_QW; ++t) s[t] = 0.f;
    const float* kr = Ks + lane * KS;
    const float* qr = Qs + (w * AED_QW) * DK;
#pragma unroll 8
    for (int e = 0; e < DK; ++e) {
      const float kv = kr[e];
#pragma unroll
      for (int t = 0; t < AED_QW; ++t) s[t] = fmaf(qr[t * DK + e], kv, s[t]);
    }
    const int key = t0 + lane;
    float p[AED_QW];
#pragma unroll
    for (int t = 0; t < AED_QW; ++t) {
      const int qi = q_lo + w * AED_QW + t;                        // the query's position among its hypothesis's rows
      const bool visible = key < kv_end && (!causal || key <= qi) && (w * AED_QW + t) < nq;
      const float sc = visible ? s[t] * scale : -INFINITY;
      const float m_new = fmaxf(m[t], wave_max(sc));
      float alpha = 1.f;
      p[t] = 0.f;
      if (m_new > -INFINITY) {                                     // wave-uniform
        alpha = expf(m[t] - m_new);                                // 0 for the first tile with a visible key
        p[t] = visible ? expf(sc - m_new) : 0.f;
      }
      l[t] = l[t] * alpha + wave_sum(p[t]);
      m[t] = m_new;
#pragma unroll
      for (int c = 0; c < DPL; ++c) o[t][c] *= alpha;
    }
    for (int j = 0; j < AED_KT; ++j) {
      float vj[DPL];
#pragma unroll
      for (int c = 0; c < DPL; ++c) vj[c] = (lane + 64 * c < DK) ? Vs[j * DK + lane + 64 * c] : 0.f;
#pragma unroll
      for (int t = 0; t < AED_QW; ++t) {
        const float pj = lane_bcast(p[t], j);
#pragma unroll
        for (int c = 0; c < DPL; ++c) o[t][c] = fmaf(pj, vj[c], o[t][c]);
      }
    }
  }

#pragma unroll
  for (int t = 0; t < AED_QW; ++t) {
    const int r = w * AED_QW + t;
    if (r >= nq) continue;
    const float inv = l[t] > 0.f ? 1.f / l[t] : 0.f;
    float* orow = out + (size_t)(q_row0 + q_lo + r) * ldo + col0;
#pragma unroll
    for (int c = 0; c < DPL; ++c)
      if (lane + 64 * c < DK) orow[lane + 64 * c] = o[t][c] * inv;
  }
}

template <int DK>
static int launch_aed_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* desc,
                                int n_slots, int max_q, int q_rows, int kv_rows, int H, float scale, float* out, int ldo,
                                hipStream_t stream) {
  constexpr size_t lds = aed_attention_lds_bytes<DK>();
  static_assert(lds <= 160 * 1024, "the K / V / Q tiles must fit one CU's LDS");
  static PerDeviceOnce once;
  if (lds > 64 * 1024 && !once.done()) {
    M3_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&aed_attention_kernel<DK>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    once.mark();
  }
  const dim3 grid((unsigned)n_slots, (unsigned)H, (unsigned)cdiv(max_q, AED_QT));
  hipLaunchKernelGGL(aed_attention_kernel<DK>, grid, dim3(256), lds, stream, q, ldq, k, ldk, v, ldv, desc, q_rows, kv_rows, scale,
                     out, ldo);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- score
// one wave per packed row: log_softmax(logits[row])[target[row]]
__global__ __launch_bounds__(256) void aed_row_logp_kernel(const float* __restrict__ logits, int ldl,
                                                           const int32_t* __restrict__ target, int rows, int V,
                                                           float* __restrict__ row_logp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* x = logits + (size_t)row * ldl;
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < V; c += 64) sum += expf(x[c] - mx);
  sum = wave_sum(sum);
  const int t = target[row];
  if (lane == 0) row_logp[row] = (t >= 0 && t < V) ? (x[t] - mx) - logf(sum) : NAN;
}

// one work-group (one wave) per utterance: lane i sums hypothesis i's rows in row order, lane 0 picks the best
__global__ __launch_bounds__(64) void aed_select_kernel(const float* __restrict__ row_logp, const float* __restrict__ r_row_logp,
                                                        const int32_t* __restrict__ hyp_row0, const int32_t* __restrict__ n_hyps,
                                                        const float* __restrict__ prior, int beam, int rows, float ctc_weight,
                                                        float reverse_weight, float* __restrict__ att, float* __restrict__ r_att,
                                                        float* __restrict__ final_score, int32_t* __restrict__ best) {
  __shared__ float fin[64];
  const int b = blockIdx.x, i = threadIdx.x;
  const int n = min(max(n_hyps[b], 0), beam);
  if (i < beam) {
    const int h = b * beam + i;
    float a = -INFINITY, r = -INFINITY, f = -INFINITY;
    const int r0 = hyp_row0[h], r1 = hyp_row0[h + 1];
    if (i < n && r0 >= 0 && r1 > r0 && r1 <= rows) {
      a = 0.f;
      for (int row = r0; row < r1; ++row) a += row_logp[row];
      f = a;
      r = 0.f;
      if (r_row_logp) {
        for (int row = r0; row < r1; ++row) r += r_row_logp[row];
        f = a * (1.f - reverse_weight) + r * reverse_weight;
      }
      if (ctc_weight != 0.f) f += prior[h] * ctc_weight;
    }
    att[h] = a;
    r_att[h] = r;
    final_score[h] = f;
    fin[i] = f;
  }
  __syncthreads();
  if (i == 0) {
    int arg = -1;
    float top = -INFINITY;
    for (int j = 0; j < n; ++j)
      if (arg < 0 || fin[j] > top) {                               // the first strictly largest (model/ctc_aed.py:249)
        arg = j;
        top = fin[j];
      }
    best[b] = arg;
  }
}

}  // namespace m3

using namespace m3;

extern "C" {

int m3_aed_embed(const int32_t* hyp_tokens, const int32_t* hyp_len, const int32_t* n_hyps, const int32_t* hyp_row0, int B,
                 int beam, int max_frames, const float* emb, const float* pe, int pe_rows, int V, int D, int reverse, int rows,
                 float* x, int ldx, int32_t* target, m3_stream stream) {
  M3_REQUIRE(B >= 0 && beam >= 1 && max_frames >= 0 && rows >= 0, "aed_embed: B=%d beam=%d max_frames=%d rows=%d", B, beam,
             max_frames, rows);
  M3_REQUIRE(V >= 1 && D >= 4 && (D & 3) == 0 && ldx >= D && pe_rows >= 1, "aed_embed: V=%d, D=%d (a multiple of 4), ldx=%d, pe_rows=%d",
             V, D, ldx, pe_rows);
  if (B == 0 || rows == 0) return 0;
  M3_REQUIRE(hyp_tokens && hyp_len && n_hyps && hyp_row0 && emb && pe && x && target, "aed_embed: null pointer");
  M3_REQUIRE((((uintptr_t)emb | (uintptr_t)pe) & 15) == 0, "aed_embed: emb / pe must be 16-byte aligned");
  hipLaunchKernelGGL(aed_embed_kernel, dim3((unsigned)(B * beam)), dim3(256), 0, (hipStream_t)stream, hyp_tokens, hyp_len, n_hyps,
                     hyp_row0, beam, max_frames, emb, pe, pe_rows, V, D, reverse, rows, sqrtf((float)D), x, ldx, target);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* att_desc,
                     int n_slots, int max_q, int q_rows, int kv_rows, int H, int dk, float scale, float* out, int ldo,
                     m3_stream stream) {
  M3_REQUIRE(n_slots >= 0 && max_q >= 0 && q_rows >= 0 && kv_rows >= 0, "aed_attention: n_slots=%d max_q=%d q_rows=%d kv_rows=%d",
             n_slots, max_q, q_rows, kv_rows);
  M3_REQUIRE(H >= 1 && H <= 65535 && dk >= 16 && dk <= 128 && dk % 16 == 0, "aed_attention: H=%d, dk=%d (a multiple of 16, <= 128)", H, dk);
  const int D = H * dk;
  M3_REQUIRE(ldq >= D && ldk >= D && ldv >= D && ldo >= D && !((ldq | ldk | ldv) & 3),
             "aed_attention: ldq=%d ldk=%d ldv=%d must be multiples of 4 and, with ldo=%d, >= H * dk = %d", ldq, ldk, ldv, ldo, D);
  if (n_slots == 0 || max_q == 0 || q_rows == 0) return 0;
  M3_REQUIRE(kv_rows >= 1, "aed_attention: no key rows (kv_len = 0 is rejected: every query needs a visible key)");
  M3_REQUIRE(q && k && v && att_desc && out, "aed_attention: null pointer");
  M3_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "aed_attention: q / k / v must be 16-byte aligned");
  M3_REQUIRE(cdiv(max_q, AED_QT) <= 65535, "aed_attention: max_q=%d too large", max_q);
  hipStream_t s = (hipStream_t)stream;
#define M3_AED_ATT(DK) \
  case DK: return launch_aed_attention<DK>(q, ldq, k, ldk, v, ldv, att_desc, n_slots, max_q, q_rows, kv_rows, H, scale, out, ldo, s)
  switch (dk) {
    M3_AED_ATT(16);
    M3_AED_ATT(32);
    M3_AED_ATT(48);
    M3_AED_ATT(64);
    M3_AED_ATT(80);
    M3_AED_ATT(96);
    M3_AED_ATT(112);
    M3_AED_ATT(128);
  }
#undef M3_AED_ATT
  m3::set_error("aed_attention: dk=%d", dk);
  return -2;
}

int m3_aed_score(const float* logits, int ldl, const float* r_logits, int ldrl, const int32_t* target, const int32_t* r_target,
                 const int32_t* hyp_row0, const int32_t* n_hyps, const float* prior, int B, int beam, int rows, int V,
                 float ctc_weight, float reverse_weight, float* row_logp, float* att, float* r_att, float* final_score,
                 int32_t* best, m3_stream stream) {
  M3_REQUIRE(B >= 0 && beam >= 1 && beam <= 64 && rows >= 0 && V >= 1, "aed_score: B=%d, beam=%d (1..64), rows=%d, V=%d", B, beam, rows, V);
  if (B == 0) return 0;
  M3_REQUIRE(hyp_row0 && n_hyps && att && r_att && final_score && best, "aed_score: null pointer");
  M3_REQUIRE(ctc_weight == 0.f || prior, "aed_score: ctc_weight = %g needs the prior scores", ctc_weight);
  hipStream_t s = (hipStream_t)stream;
  if (rows > 0) {
    M3_REQUIRE(logits && target && row_logp && ldl >= V, "aed_score: logits / target / row_logp, ldl=%d >= V=%d", ldl, V);
    M3_REQUIRE(!r_logits || (r_target && ldrl >= V), "aed_score: r_logits needs r_target and ldrl=%d >= V=%d", ldrl, V);
    hipLaunchKernelGGL(aed_row_logp_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, logits, ldl, target, rows, V, row_logp);
    M3_LAUNCH_CHECK();
    if (r_logits) {
      hipLaunchKernelGGL(aed_row_logp_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, r_logits, ldrl, r_target, rows, V,
                         row_logp + rows);
      M3_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(aed_select_kernel, dim3((unsigned)B), dim3(64), 0, s, (const float*)row_logp,
                     (const float*)(r_logits && rows > 0 ? row_logp + rows : nullptr), hyp_row0, n_hyps, prior, beam, rows, ctc_weight,
                     reverse_weight, att, r_att, final_score, best);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
