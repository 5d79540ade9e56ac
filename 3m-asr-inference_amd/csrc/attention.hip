// Fused relative-position multi-head attention (flash-style, fp32 MFMA 16x16x4).
//
// Replaces the layer chain emitted by RelPositionMultiHeadedAttention.forward
// (trainer_3m_fix/layer/attention.py:320-384) + forward_attention_trt (:199-239):
// 6 shuffles, 2 bias adds, q.k^T and q.p^T batched matmuls, add, AttMaskedSoftmax plugin
// (att_masked_softmax_kernel.cu:224-272 / common.cuh:264-360), p.v matmul, transpose+reshape --
// with the (B,h,T',T') score tensor never materialised:
//   s_ij = ((q_i + u) . k_j + (q_i + v) . p_j) * scale          (NO rel_shift, as in the reference)
//   a_ij = softmax_j(s_ij | j < len[b]),  a_ij = 0 for j >= len[b];   ctx_i = sum_j a_ij v_j
// Inputs: qkv [B*T][ldq] = (q | k | v) rows from the fused QKV projection, p [T][ldp] = linear_pos(pos_emb)
// (shared by the batch), pos_bias_u/v [h][dk].  Output ctx [B*T][ldo] with heads merged, i.e. the
// "attn_transpose_and_reshape" shuffle is folded into the store.
// One workgroup (4 waves) per (batch, head, 16-query tile): wave w walks key tiles w, w+4, ... with an
// online softmax (so a 50-frame utterance is one key tile per wave = one memory round trip), the
// probability tile goes C-layout -> A-layout through a 1 KB LDS patch per wave, and the four partial
// (max, sum, O) states are merged through LDS.  A wave's FIRST key tile skips the online-softmax rescale (its state
// is m = -inf, l = o = +0: the rescale is the identity bit for bit), so at T' <= 64 no wave rescales at all.  The merge
// (att_merge_store, shared with the chunk-by-chunk kernel) computes a row's total max, its four factors exp(m_w - m_tot) and
// its total sum once per row in every wave, and per output element only the four multiply-adds and the division.
// Per work-group the operands are 52 KB (dk = 64) / 100 KB (dk = 128) pulled by ONE CU: at T' = 50 that pull, not the
// instruction stream, is the longest phase.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kernels.h"

// -DM3_ATT_DIAG: phase stamps (s_memtime) of wave 0 of every work-group of the fp32 kernels into a debug buffer
// (tools/diag_attention.py).  No stamp executes in the normal build.
#ifdef M3_ATT_DIAG
#define M3_ADIAG(...) __VA_ARGS__
#else
#define M3_ADIAG(...)
#endif

namespace m3 {

#ifdef M3_ATT_DIAG
__device__ unsigned long long g_att_dbg[2048 * 8];
// (one statement: the wait belongs to the stamp; the fences keep the compiler from moving work across it)
__device__ __forceinline__ unsigned long long att_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
// stamps: 0 entry | 1 arguments loaded | 2 operands landed | 3 scores done | 4 softmax done | 5 P.V done | 6 barrier passed | 7 merge stored
__device__ __forceinline__ void att_diag_write(const unsigned long long (&dg)[8], int wg_id, int wave, int lane) {
  if (lane == 0 && wave == 0 && wg_id < 2048)
    for (int i = 0; i < 8; ++i) g_att_dbg[(size_t)wg_id * 8 + i] = dg[i];
}
#endif

// ---- shared by the full-utterance and the chunk-by-chunk kernel ----
// The partial O of a wave lies in LDS as [16 rows][MLD], column col of output tile n being channel 16 n + col.  MLD = dk + 4: the
// two row groups (kq, kq + 1) that share a 32-lane half of a ds_write_b32 sit 16 banks apart, columns 0..15 against 16..31; the
// merge reads 32 consecutive channels of a row.  Neither side has a bank conflict.  (A lane map with consecutive channels per
// lane -- V rows as 16-byte loads -- was built and measured: the operand phase did not move)
constexpr int att_mo_ld(int dk) { return dk + 4; }
// a load at a wave-uniform base plus a 32-bit element offset (the byte offset stays below 2^32: kAttMaxRowSpan)
template <typename V>
__device__ __forceinline__ V att_ld(const float* base, unsigned off) {
  return *reinterpret_cast<const V*>(reinterpret_cast<const char*>(base) + (off << 2));
}
// n / d as the high half of n * magic, magic = 2^32 / d + 1 (att_magic; 0 stands for d = 1): exact while n d < 2^32
__device__ __forceinline__ int att_div(int n, unsigned magic) { return magic ? (int)__umulhi((unsigned)n, magic) : n; }

// The four waves' partial (max, sum, O) states of 16 query rows -> the context rows, after the work-group's barrier.
// Per row, once: m_tot, the four factors f[w] = exp(m[w] - m_tot) (0 for a wave without a visible key) and l_tot, by lane
// (w, i) = (lane / 16, lane % 16) of EVERY wave -- redundant, but wave-private: no second barrier.  Per output element only
// acc = (((0 + O0 f0) + O1 f1) + O2 f2) + O3 f3  and the division.  dk >= 64: the 64 elements of a wave in one trip are one
// row, so the row's factors are read with v_readlane (the multiplies take them as scalar operands); below that by ds_bpermute.
// Every lane stays active up to the store: a bpermute reads nothing from an inactive lane.
template <int DK>
__device__ __forceinline__ void att_merge_store(const float (*mm)[16], const float (*ml)[16], const float* mo, int q0, int q_end,
                                                size_t brow, int h, float* __restrict__ out, int ldo, int out_bf16) {
  constexpr int MLD = att_mo_ld(DK);
  const int lane = threadIdx.x & 63, fw = lane >> 4, fi = lane & 15;
  const float m_tot = fmaxf(fmaxf(mm[0][fi], mm[1][fi]), fmaxf(mm[2][fi], mm[3][fi]));
  const float mw = mm[fw][fi];
  const float f = (mw == -INFINITY) ? 0.f : expf(mw - m_tot);   // waves without a (visible) key tile: factor 0
  const float lf = ml[fw][fi] * f;
  float l_tot = 0.f;                                            // of row fi, in every lane (w, fi)
#pragma unroll
  for (int w = 0; w < 4; ++w) l_tot += __shfl(lf, 16 * w + fi, 64);
  auto row_value = [&](float v, int src) {
    if constexpr (DK >= 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(src)));
    else return __shfl(v, src, 64);
  };
  float* orow = out + (brow * ldo + h * DK);
  bf16_t* orow16 = reinterpret_cast<bf16_t*>(out) + (brow * ldo + h * DK);
  for (int idx = threadIdx.x; idx < 16 * DK; idx += 256) {
    const int i = idx / DK, d = idx - i * DK;
    const float* mrow = mo + i * MLD + d;
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) acc += mrow[w * 16 * MLD] * row_value(f, 16 * w + i);
    const float lt = row_value(l_tot, i);
    const float o = lt > 0.f ? acc / lt : 0.f;       // a row with no visible key (padded query under a chunk mask): zeros
    const int qrow = q0 + i;
    if (qrow < q_end) {
      const unsigned off = (unsigned)qrow * (unsigned)ldo + d;
      if (out_bf16) orow16[off] = (bf16_t)o;
      else orow[off] = o;
    }
  }
}

// (the body as a device function of the work-group id: relpos_attention_dual_kernel runs two independent attention problems --
//  the embed encoder's and the main encoder's first block, different head widths -- in one launch; engine.hip "horizontal fusion")
template <int DK>
__device__ __forceinline__ void relpos_attention_body(const float* __restrict__ qkv, int ldq, const float* __restrict__ pmat, int ldp,
                                                      const float* __restrict__ pos_u, const float* __restrict__ pos_v,
                                                      const int32_t* __restrict__ row_len, int T, int D, float scale,
                                                      float* __restrict__ out, int ldo, int out_bf16, const int32_t* __restrict__ row0,
                                                      int QT, int H, int xcd_map, int chunk, int left_chunks, unsigned qt_magic, unsigned h_magic,
                                                      const int wg_id) {
  constexpr int KS = DK / 16, MLD = att_mo_ld(DK);
  M3_ADIAG(unsigned long long dg[8] = {0, 0, 0, 0, 0, 0, 0, 0}; dg[0] = att_stamp();)
  // one batch of kernel-argument loads instead of one per first use (see gemm.hip: ~5 dependent s_load rounds otherwise)
  asm volatile("" ::"s"(qkv), "s"(ldq), "s"(pmat), "s"(ldp), "s"(pos_u), "s"(pos_v), "s"(row_len), "s"(T), "s"(D), "s"(scale),
               "s"(out), "s"(ldo), "s"(out_bf16), "s"(row0), "s"(QT), "s"(H), "s"(xcd_map), "s"(chunk), "s"(left_chunks), "s"(qt_magic),
               "s"(h_magic));
  M3_ADIAG(dg[1] = att_stamp();)
  __shared__ __attribute__((aligned(16))) float ps_all[4][16][20];
  __shared__ float mo[4][16][MLD];   // per-wave partial O
  __shared__ float mm[4][16], ml[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  float (*ps)[20] = ps_all[wave];
  // work-group -> (batch, head, query tile).  The QT query tiles of one (batch, head) read the same K / V / P rows: with
  // xcd_map they get block ids that are congruent mod 8, i.e. one XCD and one L2 (blocks are dealt round-robin over the 8
  // XCDs), so those rows leave memory once instead of once per query tile (PMC: 1.55 MB -> see DESIGN.md 3).  Placement
  // only changes speed, never the result.
  int b, h, q0;
  {
    const int id = wg_id;
    int bh, qt;
    // (quotients by multiplication: att_pack's magic numbers, exact for every work-group id of the launch)
    if (xcd_map) {
      const int g = id & 7, slot = id >> 3, sq = att_div(slot, qt_magic);
      bh = sq * 8 + g;
      qt = slot - sq * QT;
    } else {
      bh = att_div(id, qt_magic);
      qt = id - bh * QT;
    }
    b = att_div(bh, h_magic);
    h = bh - b * H;
    q0 = qt * 16;
  }
  // packed rows (row0 != null): utterance b owns rows [row0[b], row0[b] + len) -- nothing beyond its last frame may be
  // read (it is another utterance's) or written; padded rows: [b T, (b+1) T), frames >= len hold defined values.
  // In the padded form brow, last and q_end come from the arguments alone: row_len[b] is requested here and waited for behind
  // the operand requests.
  int len_in = T;
  if (row_len) len_in = row_len[b];
  size_t brow = (size_t)b * T;
  int last = T - 1;                                 // clamp for the addresses of masked lanes
  int q_end = T;                                    // query rows this utterance owns
  if (row0 != nullptr) {
    const int len_p = min(__builtin_amdgcn_readfirstlane(len_in), T);
    if (q0 >= len_p) return;
    brow = (size_t)__builtin_amdgcn_readfirstlane(row0[b]);
    last = len_p - 1;
    q_end = len_p;
  }
  // this utterance's rows, this head's columns: a wave-uniform 64-bit base plus a 32-bit byte offset per lane (a row index
  // below T times a row stride: check_relpos_attention keeps T ld under 2^30 elements)
  const float* qb = qkv + brow * ldq + h * DK;      // q | k at + D | v at + 2 D
  const float* pb0 = pmat + h * DK;

  // K / P fragments of the key tile at j0, and its V fragments: B[k = key 4kq+jj][n = channel 16n+col]
  auto load_tile = [&](const int j0, f32x4 (&kb)[KS], f32x4 (&pb)[KS], float (&vb)[4][KS]) {
    const unsigned kj = (unsigned)min(j0 + col, last);
    const unsigned koff = kj * (unsigned)ldq + 4 * kq, poff = kj * (unsigned)ldp + 4 * kq;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kb[s] = att_ld<f32x4>(qb + D, koff + 16 * s);
      pb[s] = att_ld<f32x4>(pb0, poff + 16 * s);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const unsigned voff = (unsigned)min(j0 + 4 * kq + jj, last) * (unsigned)ldq + col;
#pragma unroll
      for (int n = 0; n < KS; ++n) vb[jj][n] = att_ld<float>(qb + 2 * D, voff + 16 * n);
    }
  };

  // Q and the position biases, then -- behind the additions -- the operands of the wave's first key tile (a wave without a key
  // in that tile reads clamped rows for nothing).  Requesting the tile before the wait for Q was measured and is no faster
  // (the work-group's operands arrive at the rate one CU pulls, in either order); the fence keeps the order measured.
  f32x4 qu[KS], qv[KS], kb[KS], pb[KS];
  float vb[4][KS];
  {
    const unsigned qoff = (unsigned)min(q0 + col, last) * (unsigned)ldq + 4 * kq;
    f32x4 q4[KS], pu[KS], pv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      q4[s] = att_ld<f32x4>(qb, qoff + 16 * s);
      pu[s] = ldg4(pos_u + h * DK + 16 * s + 4 * kq);
      pv[s] = ldg4(pos_v + h * DK + 16 * s + 4 * kq);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qu[s] = q4[s] + pu[s];
      qv[s] = q4[s] + pv[s];
    }
    __builtin_amdgcn_sched_barrier(0);
    load_tile(16 * wave, kb, pb, vb);
  }
  f32x4 o[KS];
#pragma unroll
  for (int n = 0; n < KS; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -INFINITY;
    l_run[r] = 0.f;
  }

  // static chunk mask (utils/mask.py:42-75 subsequent_chunk_mask, :127-134 static_chunk_size): query i sees keys
  // [max((i / chunk - left_chunks) chunk, 0), min((i / chunk + 1) chunk, T)) -- all left chunks when left_chunks < 0 --
  // besides the padding mask key < len.  chunk <= 0: full context.  Rows of this lane's accumulators: 4 kq + r.
  const int len = min(__builtin_amdgcn_readfirstlane(len_in), T);
  int klo[4], khi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + 4 * kq + r;
    klo[r] = 0;
    khi[r] = len;
    if (chunk > 0) {
      const int c = qrow / chunk;
      klo[r] = left_chunks < 0 ? 0 : max((c - left_chunks) * chunk, 0);
      khi[r] = min(min((c + 1) * chunk, T), len);
    }
  }
  // One key tile: scores (the alternating K / P chain), online softmax, P.V.  FIRST: the wave's first tile.  Its state is
  // m_run = -inf, l_run = +0, o = +0, so the rescale is the identity bit for bit and is left out: corr is 1 or expf(-inf) = +0,
  // (+0) corr = +0, and (+0) + s = s for the sum s >= 0 of the probabilities.  At T' <= 64 that is the only tile of every wave.
  auto run_tile = [&](auto first, const int j0) {
    constexpr bool FIRST = decltype(first)::value;
    M3_ADIAG(if (FIRST) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); dg[2] = att_stamp(); })
    f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc = mfma16(qu[s][j], kb[s][j], sc);
        sc = mfma16(qv[s][j], pb[s][j], sc);
      }
    M3_ADIAG(if (FIRST) { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); dg[3] = att_stamp(); })
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = (j0 + col) >= klo[r] && (j0 + col) < khi[r];
      const float sv = valid ? sc[r] * scale : -INFINITY;
      const float m_new = fmaxf(m_run[r], group16_max(sv));
      const float pexp = valid ? expf(sv - m_new) : 0.f;
      if constexpr (FIRST) {
        l_run[r] = group16_sum(pexp);
      } else {
        const float corr = (m_new == -INFINITY) ? 1.f : expf(m_run[r] - m_new);   // (a key tile wholly outside the row's chunk window)
        l_run[r] = l_run[r] * corr + group16_sum(pexp);
#pragma unroll
        for (int n = 0; n < KS; ++n) o[n][r] *= corr;
      }
      m_run[r] = m_new;
      ps[4 * kq + r][col] = pexp;
    }
    M3_ADIAG(if (FIRST) dg[4] = att_stamp();)
    // ps is private to this wave and a wave's LDS operations execute in order: only the compiler has
    // to be kept from moving the transposed read across the writes (no s_barrier needed)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f32x4 pa = *reinterpret_cast<const f32x4*>(&ps[col][4 * kq]);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int n = 0; n < KS; ++n)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) o[n] = mfma16(pa[jj], vb[jj][n], o[n]);
    M3_ADIAG(if (FIRST) { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); dg[5] = att_stamp(); })
  };
  if (16 * wave < len) {
    run_tile(std::true_type{}, 16 * wave);
    for (int j0 = 16 * wave + 64; j0 < len; j0 += 64) {
      load_tile(j0, kb, pb, vb);
      run_tile(std::false_type{}, j0);
    }
  }

  // ---- merge the four waves' partial softmax states ----
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (col == 0) {
      mm[wave][4 * kq + r] = m_run[r];
      ml[wave][4 * kq + r] = l_run[r];
    }
#pragma unroll
    for (int n = 0; n < KS; ++n) mo[wave][4 * kq + r][16 * n + col] = o[n][r];
  }
  __syncthreads();
  M3_ADIAG(dg[6] = att_stamp();)
  att_merge_store<DK>(mm, ml, &mo[0][0][0], q0, q_end, brow, h, out, ldo, out_bf16);
  M3_ADIAG(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); dg[7] = att_stamp(); att_diag_write(dg, wg_id, wave, lane);)
}

// One record per problem, filled by att_pack: the single kernel takes one, the dual kernel two.  QT, the XCD mapping and the
// work-group count are derived there, once.
struct AttKernArgs {
  const float *qkv; int ldq; const float* pmat; int ldp; const float *pos_u, *pos_v; const int32_t* row_len; int T, D; float scale;
  float* out; int ldo, out_bf16; const int32_t* row0; int QT, H, xcd_map, chunk, left_chunks; unsigned qt_magic, h_magic; int n_wg;
};
#define M3_ATT_SPREAD(a) a.qkv, a.ldq, a.pmat, a.ldp, a.pos_u, a.pos_v, a.row_len, a.T, a.D, a.scale, a.out, a.ldo, a.out_bf16, a.row0, a.QT, a.H, a.xcd_map, a.chunk, a.left_chunks, a.qt_magic, a.h_magic
template <int DK>
__global__ __launch_bounds__(256) void relpos_attention_kernel(const AttKernArgs a) {
  relpos_attention_body<DK>(M3_ATT_SPREAD(a), (int)blockIdx.x);
}
// work-groups [0, n0) the first problem (n0 = its count rounded up to a multiple of 8: "id % 8 = XCD" holds for both), the rest the second
template <int DK0, int DK1>
__global__ __launch_bounds__(256) void relpos_attention_dual_kernel(const AttKernArgs a, const AttKernArgs b, const int n0) {
  if ((int)blockIdx.x < n0) {
    if ((int)blockIdx.x < a.n_wg) relpos_attention_body<DK0>(M3_ATT_SPREAD(a), (int)blockIdx.x);
  } else {
    relpos_attention_body<DK1>(M3_ATT_SPREAD(b), (int)blockIdx.x - n0);
  }
}
#undef M3_ATT_SPREAD


// ------------------------------------------------------------------------------------------------------------------------
// Chunk-by-chunk (streaming) form: the queries are the C frames of the current chunk, the keys / values are every frame the
// static chunk mask lets them see -- the chunk itself (still in the QKV GEMM's output) and the frames to its left, which come
// from the per-layer history `hist` [B][cap][2 D] (K | V rows of all earlier chunks, a ring when cap < the stream's length).
// This is what the reference's cache plugins were written for: CatSplitCachePluginDynamic concatenates the cached K / V with
// the chunk's and splits the new cache off (cat_split_cache_kernel.cu:30-107), AttStreamSoftmaxPluginDynamic masks the scores
// to [ld - decode_frame_num, mask_idx + cache_len) (att_stream_softmax_kernel.cu:136-191), RelPositionalEncoding's streaming
// form takes pe[offset : offset + T] (rel_positional_encoding_kernel.cu:108-123).  Here they are one kernel: nothing is
// concatenated or copied, the work-group that owns 16 query frames of a head also appends that head's K / V rows of those
// frames to the history (read only by LATER chunks: keys of the current chunk are taken from the QKV buffer), and p is
// indexed by the key's absolute position.  The chunk counter lives on the device (`step`), so the launch is replayable from
// a hipGraph.  Key tiles sit at absolute multiples of 16 and wave w owns tiles w, w + 4, ... exactly as in the full-utterance
// kernel above; tiles left of every row's window are skipped (there they leave the softmax state untouched), so a chunk's
// context equals the rows the full-utterance kernel computes under the same static chunk mask bit for bit.
// SLOTS (slot mode, m3_engine_forward_chunk_slots): `step` is an array, one chunk counter per utterance slot, and a slot that
// is not live in this chunk (stream_slot_live: nothing to decode, or its chunk would end past max_frames) appends nothing,
// sees no key and gets zero context rows -- no address is formed from a counter that failed the test.  The lockstep
// instantiation (SLOTS = false) is the kernel as it was: max_chunks is never read there.
template <int DK, bool SLOTS = false>
__global__ __launch_bounds__(256) void relpos_attention_stream_kernel(const float* __restrict__ qkv, int ldq,
                                                                     float* __restrict__ hist, int cap,
                                                                     const float* __restrict__ pmat, int ldp,
                                                                     const float* __restrict__ pos_u, const float* __restrict__ pos_v,
                                                                     const int32_t* __restrict__ chunk_len, const int32_t* __restrict__ step,
                                                                     int C, int D, float scale, float* __restrict__ out, int ldo,
                                                                     int QT, int H, int left_chunks, int max_chunks) {
  constexpr int KS = DK / 16;
  asm volatile("" ::"s"(qkv), "s"(ldq), "s"(hist), "s"(cap), "s"(pmat), "s"(ldp), "s"(pos_u), "s"(pos_v), "s"(chunk_len), "s"(step),
               "s"(C), "s"(D), "s"(scale), "s"(out), "s"(ldo), "s"(QT), "s"(H), "s"(left_chunks));
  __shared__ __attribute__((aligned(16))) float ps_all[4][16][20];
  __shared__ float mo[4][16][att_mo_ld(DK)];
  __shared__ float mm[4][16], ml[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  float (*ps)[20] = ps_all[wave];
  const int bh = blockIdx.x / QT, qt = blockIdx.x - bh * QT;
  const int b = bh / H, h = bh - b * H, q0 = qt * 16;
  bool slot_live = true;
  int pos = 0;
  if (SLOTS) {
    pos = step[b];
    slot_live = stream_slot_live(chunk_len[b], pos, max_chunks);
    if (!slot_live) pos = 0;
  } else {
    pos = *step;
  }
  const int off = pos * C;                                // absolute index of the chunk's first frame
  const int nlive = slot_live ? min(max(chunk_len[b], 0), C) : 0;   // valid frames of utterance b in this chunk
  const int len = off + nlive;                            // keys the utterance has so far
  const size_t brow = (size_t)b * C;
  const float* hb = hist + (size_t)b * cap * 2 * D;

  // ---- this work-group's share of the history append: K | V of head h, frames q0 .. q0 + 15 of the chunk ----
  for (int idx = threadIdx.x; idx < 16 * 2 * (DK / 4); idx += 256) {
    const int r = idx / (2 * (DK / 4)), rem = idx - r * 2 * (DK / 4), kv = rem / (DK / 4), c4 = (rem - kv * (DK / 4)) * 4;
    if (q0 + r < C && slot_live) {
      const f32x4 val = ldg4(qkv + (brow + q0 + r) * ldq + (1 + kv) * D + h * DK + c4);
      stg4(hist + ((size_t)b * cap + (size_t)((off + q0 + r) % cap)) * 2 * D + kv * D + h * DK + c4, val);
    }
  }

  const int qi = min(q0 + col, C - 1);
  const float* qrow = qkv + (brow + qi) * ldq + h * DK + 4 * kq;
  f32x4 qu[KS], qv[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const f32x4 q4 = ldg4(qrow + 16 * s);
    qu[s] = q4 + ldg4(pos_u + h * DK + 16 * s + 4 * kq);
    qv[s] = q4 + ldg4(pos_v + h * DK + 16 * s + 4 * kq);
  }
  f32x4 o[KS];
#pragma unroll
  for (int n = 0; n < KS; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -INFINITY;
    l_run[r] = 0.f;
  }
  // every query of the chunk sits in chunk number *step: one window [klo, khi) for all of them
  const int cidx = off / C;
  const int klo = left_chunks < 0 ? 0 : max((cidx - left_chunks) * C, 0);
  const int khi = min((cidx + 1) * C, len);
  const int last = max(len - 1, 0);
  for (int j0 = 16 * wave; j0 < len; j0 += 64) {
    if (j0 + 16 <= klo) continue;                          // wholly left of the window: the full kernel's state is untouched there
    const int kj = min(j0 + col, last);
    const float* krow = (kj >= off ? qkv + (brow + kj - off) * ldq + D : hb + (size_t)(kj % cap) * 2 * D) + h * DK + 4 * kq;
    const float* prow = pmat + (size_t)kj * ldp + h * DK + 4 * kq;
    f32x4 kb[KS], pb[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kb[s] = ldg4(krow + 16 * s);
      pb[s] = ldg4(prow + 16 * s);
    }
    float vb[KS][4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int vj = min(j0 + 4 * kq + jj, last);
      const float* vrow = (vj >= off ? qkv + (brow + vj - off) * ldq + 2 * D : hb + (size_t)(vj % cap) * 2 * D + D) + h * DK + col;
#pragma unroll
      for (int n = 0; n < KS; ++n) vb[n][jj] = vrow[16 * n];
    }
    f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc = mfma16(qu[s][j], kb[s][j], sc);
        sc = mfma16(qv[s][j], pb[s][j], sc);
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = (j0 + col) >= klo && (j0 + col) < khi;
      const float sv = valid ? sc[r] * scale : -INFINITY;
      const float m_new = fmaxf(m_run[r], group16_max(sv));
      const float pexp = valid ? expf(sv - m_new) : 0.f;
      const float corr = (m_new == -INFINITY) ? 1.f : expf(m_run[r] - m_new);
      l_run[r] = l_run[r] * corr + group16_sum(pexp);
      m_run[r] = m_new;
#pragma unroll
      for (int n = 0; n < KS; ++n) o[n][r] *= corr;
      ps[4 * kq + r][col] = pexp;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f32x4 pa = *reinterpret_cast<const f32x4*>(&ps[col][4 * kq]);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int n = 0; n < KS; ++n)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) o[n] = mfma16(pa[jj], vb[n][jj], o[n]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (col == 0) {
      mm[wave][4 * kq + r] = m_run[r];
      ml[wave][4 * kq + r] = l_run[r];
    }
#pragma unroll
    for (int n = 0; n < KS; ++n) mo[wave][4 * kq + r][16 * n + col] = o[n][r];
  }
  __syncthreads();
  att_merge_store<DK>(mm, ml, &mo[0][0][0], q0, C, brow, h, out, ldo, 0);
}

// (a.T: the C frames of a chunk, a.row_len: their valid count per utterance; checked by check_relpos_attention)
static int launch_relpos_attention_stream(const AttArgs& a, hipStream_t stream) {
  const int QT = cdiv(a.T, 16), D = a.H * a.dk;
  dim3 grid(QT * a.H * a.B);
  // slot_max_chunks >= 0: slot mode, `step` holds B counters (one per utterance slot)
#define M3_ATT_CASE(DK_)                                                                                                                   \
  if (a.slot_max_chunks >= 0)                                                                                                              \
    hipLaunchKernelGGL((relpos_attention_stream_kernel<DK_, true>), grid, dim3(256), 0, stream, (const float*)a.qkv, a.ldq, a.hist, a.cap, \
                       a.pmat, a.ldp, a.pos_u, a.pos_v, a.row_len, a.step, a.T, D, a.scale, (float*)a.out, a.ldo, QT, a.H, a.left_chunks,  \
                       a.slot_max_chunks);                                                                                                 \
  else                                                                                                                                     \
    hipLaunchKernelGGL((relpos_attention_stream_kernel<DK_, false>), grid, dim3(256), 0, stream, (const float*)a.qkv, a.ldq, a.hist, a.cap, \
                       a.pmat, a.ldp, a.pos_u, a.pos_v, a.row_len, a.step, a.T, D, a.scale, (float*)a.out, a.ldo, QT, a.H, a.left_chunks, 0)
  switch (a.dk) {
    case 16: M3_ATT_CASE(16); break;
    case 32: M3_ATT_CASE(32); break;
    case 64: M3_ATT_CASE(64); break;
    default: M3_ATT_CASE(128);
  }
#undef M3_ATT_CASE
  M3_LAUNCH_CHECK();
  return 0;
}


// ------------------------------------------------------------------------------------------------------------------------
// The same operator on bf16 rows for the 16-bit modes of long batches (qkv written as bf16 by the QKV GEMM, context
// written as bf16 for the output projection), T' <= 128 keys:  v_mfma_f32_16x16x32_bf16, fp32 softmax.
//
// One work-group per (utterance, head) instead of one per (utterance, head, 16-query tile): K, P = linear_pos(pos_emb) and
// V of the head are staged ONCE into LDS (full-line loads; the fp32 kernel above re-reads them per query tile and loads V
// with 4-byte accesses), then each wave takes query tiles.  Scores are computed TRANSPOSED, S^T = K (q+u)^T + P (q+v)^T
// (keys on the MFMA row axis): a lane then holds, for ITS query (column), 4 consecutive keys per 16-key tile in registers --
// the whole row of probabilities for T' <= 128 is 32 registers, softmax needs no online rescaling and no LDS transpose, and
// two key tiles packed together ARE the B operand of  O^T = V^T P^T  (k index j < 4: tile 2c key 4kq+j, j >= 4: tile 2c+1);
// V is kept transposed in LDS ([channel][key]) so that the matching A operand is two 8-byte reads.
namespace {
constexpr int kAttTP = 128;                                    // keys a work-group can hold
template <int DK> constexpr int att16_lds_bytes() { return 2 * kAttTP * (DK + 8) * 2 + DK * (kAttTP + 8) * 2; }
}  // namespace

template <int DK>
__global__ __launch_bounds__(256) void relpos_attention_bf16_kernel(const bf16_t* __restrict__ qkv, int ldq,
                                                                   const float* __restrict__ pmat, int ldp,
                                                                   const float* __restrict__ pos_u,
                                                                   const float* __restrict__ pos_v,
                                                                   const int32_t* __restrict__ row_len, int T, int D, int H,
                                                                   float scale, bf16_t* __restrict__ out, int ldo,
                                                                   const int32_t* __restrict__ row0, int chunk, int left_chunks) {
  constexpr int KLD = DK + 8;                                  // bf16 elements per K / P row in LDS (conflict-free 16-B fragment reads)
  constexpr int VLD = kAttTP + 8;                              // bf16 elements per Vt row (one channel, all keys)
  constexpr int KS = DK / 32;                                  // 32-deep k-steps of the score products
  constexpr int NCH = DK / 16;                                 // 16-channel tiles of the output
  extern __shared__ __attribute__((aligned(16))) unsigned char att_lds[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(att_lds);             // [kAttTP][KLD]
  bf16_t* Ps = Ks + kAttTP * KLD;                              // [kAttTP][KLD]
  bf16_t* Vt = Ps + kAttTP * KLD;                              // [DK][VLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int len = min(row_len ? row_len[b] : T, T);
  if (len <= 0) return;
  const size_t brow = row0 ? (size_t)row0[b] : (size_t)b * T;
  const int q_end = row0 ? len : T;                            // query rows this utterance owns (padded layout: all T)
  const int nkt = (len + 15) >> 4;                             // 16-key tiles with at least one valid key
  const int nk32 = ((len + 31) >> 5) << 5;                     // keys rounded up to the pairs the P.V product consumes

  // ---- all loads of the work-group are issued up front, clamped instead of branched (a load under a branch is one memory
  //      round trip per loop iteration): the query rows of this wave's (at most two) tiles, then K / P / V of the head ----
  constexpr int QT = kAttTP / 64;                              // query tiles per wave
  bf16x8 q8[QT][KS];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int qi = min(16 * wave + 64 * i + col, q_end - 1);
    const bf16_t* qrow = qkv + (brow + qi) * ldq + h * DK + 8 * kq;
#pragma unroll
    for (int s = 0; s < KS; ++s) q8[i][s] = *reinterpret_cast<const bf16x8*>(qrow + 32 * s);
  }
  f32x4 pu[KS][2], pv[KS][2];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    pu[s][0] = ldg4(pos_u + h * DK + 32 * s + 8 * kq);
    pu[s][1] = ldg4(pos_u + h * DK + 32 * s + 8 * kq + 4);
    pv[s][0] = ldg4(pos_v + h * DK + 32 * s + 8 * kq);
    pv[s][1] = ldg4(pos_v + h * DK + 32 * s + 8 * kq + 4);
  }
  {
    constexpr int CPR = DK / 8;                                // 16-byte chunks per row
    constexpr int RPP = 256 / CPR;                             // rows per pass
    constexpr int NP = kAttTP / RPP;                           // passes over the key rows
    const int c = tid % CPR, r0 = tid / CPR;
    u32x4 kv[NP], vv[NP];
    f32x4 p0[NP], p1[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int j = min(r0 + RPP * i, len - 1);                // keys >= len: a valid row is read and replaced by zeros below
      const bf16_t* rowp = qkv + (brow + j) * ldq + h * DK + 8 * c;
      kv[i] = *reinterpret_cast<const u32x4*>(rowp + D);
      vv[i] = *reinterpret_cast<const u32x4*>(rowp + 2 * D);
      const float* pr = pmat + (size_t)j * ldp + h * DK + 8 * c;
      p0[i] = ldg4(pr);
      p1[i] = ldg4(pr + 4);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int j = r0 + RPP * i;
      if (j < nk32) {
        const bool on = j < len;
        *reinterpret_cast<u32x4*>(Ks + j * KLD + 8 * c) = on ? kv[i] : u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<bf16x8*>(Ps + j * KLD + 8 * c) = cvt8(on ? p0[i] : f32x4{0.f, 0.f, 0.f, 0.f}, on ? p1[i] : f32x4{0.f, 0.f, 0.f, 0.f});
        const bf16x8 v8 = __builtin_bit_cast(bf16x8, on ? vv[i] : u32x4{0u, 0u, 0u, 0u});
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(8 * c + e) * VLD + j] = v8[e];
      }
    }
  }
  __syncthreads();

  // ---- query tiles: wave w takes tiles w and w + 4 ----
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int q0 = 16 * wave + 64 * i;
    if (q0 >= q_end) break;
    bf16x8 qu[KS], qv[KS];                                     // B operands: (q + u)^T, (q + v)^T -- lane (query col, k = 8 kq + j)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qu[s][j] = (bf16_t)((float)q8[i][s][j] + pu[s][0][j]);
        qu[s][4 + j] = (bf16_t)((float)q8[i][s][4 + j] + pu[s][1][j]);
        qv[s][j] = (bf16_t)((float)q8[i][s][j] + pv[s][0][j]);
        qv[s][4 + j] = (bf16_t)((float)q8[i][s][4 + j] + pv[s][1][j]);
      }
    }
    // static chunk mask (see the fp32 kernel): this lane's query sees keys [klo, khi)
    int klo = 0, khi = len;
    if (chunk > 0) {
      const int c = (q0 + col) / chunk;
      klo = left_chunks < 0 ? 0 : max((c - left_chunks) * chunk, 0);
      khi = min(min((c + 1) * chunk, T), len);
    }
    // scores, transposed: sT[t][r] = s(query col, key 16 t + 4 kq + r)
    f32x4 sT[kAttTP / 16];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < kAttTP / 16; ++t) {
      sT[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < nkt) {
        const bf16_t* krow = Ks + (16 * t + col) * KLD + 8 * kq;
        const bf16_t* prow = Ps + (16 * t + col) * KLD + 8 * kq;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          sT[t] = mfma16h(*reinterpret_cast<const bf16x8*>(krow + 32 * s), qu[s], sT[t]);
          sT[t] = mfma16h(*reinterpret_cast<const bf16x8*>(prow + 32 * s), qv[s], sT[t]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * kq + r;
        const bool valid = key >= klo && key < khi;
        sT[t][r] = valid ? sT[t][r] * scale : -INFINITY;
        mx = fmaxf(mx, sT[t][r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));                    // the four key quarters of this query's column
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
    const float mref = mx == -INFINITY ? 0.f : mx;            // (no visible key at all: a padded query under a chunk mask)
#pragma unroll
    for (int t = 0; t < kAttTP / 16; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sT[t][r] = __expf(sT[t][r] - mref);                    // masked keys: exp(-inf) = 0
        sum += sT[t][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
    // O^T = V^T P^T over pairs of key tiles
    f32x4 oT[NCH];
#pragma unroll
    for (int n = 0; n < NCH; ++n) oT[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c2 = 0; c2 < kAttTP / 32; ++c2) {
      if (2 * c2 < nkt) {
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pb[j] = (bf16_t)sT[2 * c2][j];
          pb[4 + j] = (bf16_t)sT[2 * c2 + 1][j];
        }
#pragma unroll
        for (int n = 0; n < NCH; ++n) {
          const bf16_t* vrow = Vt + (16 * n + col) * VLD + 32 * c2 + 4 * kq;
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow), hi = *reinterpret_cast<const bf16x4*>(vrow + 16);
          bf16x8 va;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            va[j] = lo[j];
            va[4 + j] = hi[j];
          }
          oT[n] = mfma16h(va, pb, oT[n]);
        }
      }
    }
    // oT[n][r] = O(query col, channel 16 n + 4 kq + r): 4 consecutive channels per lane
    const int qrow_out = q0 + col;
    if (qrow_out < q_end) {
      bf16_t* orow = out + (brow + qrow_out) * ldo + h * DK + 4 * kq;
#pragma unroll
      for (int n = 0; n < NCH; ++n) {
        bf16x4 o4;
#pragma unroll
        for (int r = 0; r < 4; ++r) o4[r] = (bf16_t)(oT[n][r] * inv);
        *reinterpret_cast<bf16x4*>(orow + 16 * n) = o4;
      }
    }
  }
}

bool relpos_attention_bf16_supports(int T, int dk) { return T <= kAttTP && (dk == 64 || dk == 128); }

int init_relpos_attention_bf16_kernels() {
  static PerDeviceOnce once;
  if (once.done()) return 0;
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)relpos_attention_bf16_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, att16_lds_bytes<64>()));
  M3_CHECK_HIP(hipFuncSetAttribute((const void*)relpos_attention_bf16_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, att16_lds_bytes<128>()));
  once.mark();
  return 0;
}

static int launch_relpos_attention_bf16(const AttArgs& a, hipStream_t stream) {
  if (int rc = init_relpos_attention_bf16_kernels()) return rc;
  const int D = a.H * a.dk;
#define M3_ATT_CASE(DK_)                                                                                                                       \
  hipLaunchKernelGGL((relpos_attention_bf16_kernel<DK_>), dim3(a.B * a.H), dim3(256), att16_lds_bytes<DK_>(), stream, (const bf16_t*)a.qkv, a.ldq, \
                     a.pmat, a.ldp, a.pos_u, a.pos_v, a.row_len, a.T, D, a.H, a.scale, (bf16_t*)a.out, a.ldo, a.row0, a.chunk, a.left_chunks)
  if (a.dk == 64) M3_ATT_CASE(64);
  else M3_ATT_CASE(128);
#undef M3_ATT_CASE
  M3_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// The host side of the three cores: one record (AttArgs), one check, one launcher; att_pack serves the fp32 single and dual kernels.
// the kernel's divisions by QT and H as multiplications (att_div): floor(2^32 / d) + 1, exact for n d < 2^32 -- n < the work-group
// count, which check_relpos_attention bounds; 0 marks d = 1
static unsigned att_magic(int d) { return d == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)d + 1); }
static AttKernArgs att_pack(const AttArgs& q) {
  AttKernArgs k;
  k.qkv = (const float*)q.qkv; k.ldq = q.ldq; k.pmat = q.pmat; k.ldp = q.ldp; k.pos_u = q.pos_u; k.pos_v = q.pos_v; k.row_len = q.row_len; k.T = q.T;
  k.D = q.H * q.dk; k.scale = q.scale; k.out = (float*)q.out; k.ldo = q.ldo; k.out_bf16 = q.out_bf16; k.row0 = q.row0; k.QT = cdiv(q.T, 16); k.H = q.H;
  k.xcd_map = ((q.H * q.B) % 8 == 0) ? 1 : 0; k.chunk = q.chunk; k.left_chunks = q.left_chunks; k.n_wg = k.QT * q.H * q.B;
  k.qt_magic = att_magic(k.QT); k.h_magic = att_magic(q.H);
  return k;
}
static bool att_dk(int dk) { return dk == 16 || dk == 32 || dk == 64 || dk == 128; }
constexpr size_t kAttMaxRowSpan = (size_t)1 << 30;   // elements: 32-bit byte offsets within one utterance's rows
static bool att_dual_dk(int dk) { return dk == 64 || dk == 128; }

// the three cores' argument checks (fp32 rows, bf16 rows, chunk-by-chunk), for the single and the dual launcher
static int check_relpos_attention(const AttArgs& a, bool say = true) {
  if (a.streaming) {
    M3_REQUIRE_SAY(say, a.B > 0 && a.T > 0 && a.H > 0 && a.cap >= a.T, "attention (stream): empty problem or history shorter than a chunk");
    M3_REQUIRE_SAY(say, a.left_chunks < 0 || a.cap >= (a.left_chunks + 1) * a.T, "attention (stream): a history of %d frames cannot hold %d left chunks of %d",
                   a.cap, a.left_chunks, a.T);
    M3_REQUIRE_SAY(say, (a.ldq & 3) == 0 && (a.ldp & 3) == 0 && (a.dk & 3) == 0, "attention (stream): row strides must be multiples of 4");
    M3_REQUIRE_SAY(say, a.hist && a.row_len && a.step, "attention (stream): null state");
    M3_REQUIRE_SAY(say, att_dk(a.dk), "attention (stream): d_k=%d unsupported (16/32/64/128)", a.dk);
    M3_REQUIRE_SAY(say, (size_t)a.T * (size_t)a.ldo < kAttMaxRowSpan, "attention (stream): a chunk's rows span %zu elements (limit 2^30)", (size_t)a.T * (size_t)a.ldo);
    return 0;
  }
  M3_REQUIRE_SAY(say, a.B > 0 && a.T > 0 && a.H > 0, "attention: empty problem");
  if (a.rows_bf16) {
    M3_REQUIRE_SAY(say, relpos_attention_bf16_supports(a.T, a.dk), "attention (bf16 rows): T'=%d > %d keys or d_k=%d not 64 / 128", a.T, kAttTP, a.dk);
    M3_REQUIRE_SAY(say, (a.ldq & 7) == 0 && (a.ldp & 3) == 0 && (a.ldo & 3) == 0, "attention (bf16 rows): row strides must be multiples of 8 / 4 / 4");
    return 0;
  }
  M3_REQUIRE_SAY(say, (a.ldq & 3) == 0 && (a.ldp & 3) == 0, "attention: row strides must be multiples of 4");
  M3_REQUIRE_SAY(say, att_dk(a.dk), "attention: d_k=%d unsupported (16/32/64/128)", a.dk);
  // the kernel adds a 32-bit byte offset (a row below T' times a row stride) to an utterance's 64-bit base
  const size_t span = (size_t)a.T * (size_t)std::max(std::max(a.ldq, a.ldp), a.ldo);
  const size_t n_wg = (size_t)cdiv(a.T, 16) * a.H * a.B;       // (the ids divided by QT and by H in the kernel: att_div)
  M3_REQUIRE_SAY(say, n_wg * (size_t)std::max(cdiv(a.T, 16), a.H) < ((size_t)1 << 32), "attention: %zu work-groups are more than the kernel's id arithmetic holds", n_wg);
  M3_REQUIRE_SAY(say, span < kAttMaxRowSpan, "attention: the rows of one utterance span %zu elements (T' times the largest row stride; limit 2^30)", span);
  return 0;
}

int launch_relpos_attention(const AttArgs& a, hipStream_t stream) {
  if (int rc = check_relpos_attention(a)) return rc;
  if (a.streaming) return launch_relpos_attention_stream(a, stream);
  if (a.rows_bf16) return launch_relpos_attention_bf16(a, stream);
  const AttKernArgs k = att_pack(a);
#define M3_ATT_CASE(DK_) hipLaunchKernelGGL((relpos_attention_kernel<DK_>), dim3(k.n_wg), dim3(256), 0, stream, k)
  switch (a.dk) {
    case 16: M3_ATT_CASE(16); break;
    case 32: M3_ATT_CASE(32); break;
    case 64: M3_ATT_CASE(64); break;
    default: M3_ATT_CASE(128);
  }
#undef M3_ATT_CASE
  M3_LAUNCH_CHECK();
  return 0;
}
// two independent fp32 attention problems, head widths 64 or 128 each, in ONE launch
bool relpos_attention_dual_fusable(const AttArgs& a, const AttArgs& b) {
  return check_relpos_attention(a, false) == 0 && check_relpos_attention(b, false) == 0 && !a.streaming && !b.streaming && !a.rows_bf16 &&
         !b.rows_bf16 && att_dual_dk(a.dk) && att_dual_dk(b.dk);
}
int launch_relpos_attention_dual(const AttArgs& a, const AttArgs& b, hipStream_t stream) {
  M3_REQUIRE(relpos_attention_dual_fusable(a, b), "attention dual: head widths %d / %d are not a dual instantiation", a.dk, b.dk);
  const AttKernArgs ka = att_pack(a), kb = att_pack(b);
  const int n0 = (int)align_up((size_t)ka.n_wg, 8);
  dim3 grid(n0 + kb.n_wg);
#define M3_ATTD(D0_, D1_) hipLaunchKernelGGL((relpos_attention_dual_kernel<D0_, D1_>), grid, dim3(256), 0, stream, ka, kb, n0)
  if (a.dk == 128 && b.dk == 64) M3_ATTD(128, 64);
  else if (a.dk == 64 && b.dk == 128) M3_ATTD(64, 128);
  else if (a.dk == 64) M3_ATTD(64, 64);
  else M3_ATTD(128, 128);
#undef M3_ATTD
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3

#ifdef M3_ATT_DIAG
extern "C" int m3_debug_att_read(void* dst, size_t bytes) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(m3::g_att_dbg), bytes < sizeof(m3::g_att_dbg) ? bytes : sizeof(m3::g_att_dbg));
}
#endif
