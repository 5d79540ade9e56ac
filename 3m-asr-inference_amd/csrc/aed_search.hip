// Attention decoding: the AED decoder searching on its own, one new token per hypothesis per step.  These are
// the kernels a step needs besides the dense GEMMs (m3_linear): the input row of every hypothesis, ONE single-query attention
// core for self- and source attention, and the step's log-softmax / top-k / prune / bookkeeping.  R = B * beam hypothesis rows,
// row r = u * beam + slot.  Everything that changes from step to step -- position, who is finished, which utterance is done
// -- lives in the state blob, so a step is the same launches with the same arguments every time.
//
//   state (int32 words):  [ B headers of AS_HDR words: step, limit, done, mem_row0, mem_len ]
//                         [ R rows of 2 records (double buffer); record = score, finished, tokens[P], path[P] ],  P = max_steps + 1
//   utterance u at step s reads record s & 1 of its rows and (m3_aed_search_prune) writes the other one, then moves its step.
//   tokens[0] = sos, tokens[t] the t-th token; path[t] = the slot that wrote position t of this hypothesis's self-attention
//   keys, so pruning copies small integer paths and the K / V cache [layer][position][R][2D] is written once and never moved.
//
// fp32 throughout, no atomics, every reduction in a fixed order, a row's result independent of its place in the batch.  A word
// has one writer per launch, and no work-group reads a word that another work-group writes in the same launch: the step
// counters are per utterance, and the records are double-buffered.
#include "aed_search_state.h"   // the state layout and the pick order, shared with aed_joint.hip

namespace m3 {
namespace {

size_t search_cache_bytes(const m3_aed_search_desc* d) {
  return (size_t)d->layers * d->max_steps * ((size_t)d->B * d->beam) * 2 * d->D * sizeof(float);
}

// ---------------------------------------------------------------------------------------------------------------- reset
// one work-group per row (clears both records, then the start: [sos], slot 0 scores 0, the others -inf); slot 0's group also
// writes the utterance's header.  Record 1 is left all zero (score 0, token 0): step 0 reads record 0 only, and the first prune
// writes every word of record 1 that a later launch reads.
__global__ __launch_bounds__(64) void aed_search_reset_kernel(int32_t* state, int B, int N, int rec_words, int V, int pe_rows,
                                                              int step_cap, const int32_t* __restrict__ mem_row0,
                                                              const int32_t* __restrict__ mem_len) {
  const int r = blockIdx.x, u = r / N, slot = r - u * N, tid = threadIdx.x;
  int32_t* rec = const_cast<int32_t*>(as_record(state, B, rec_words, r, 0));
  for (int i = tid; i < 2 * rec_words; i += 64) {
    int32_t v = 0;
    if (i == AS_SCORE) v = __builtin_bit_cast(int32_t, slot == 0 ? 0.f : -INFINITY);
    if (i == AS_TOKENS) v = V - 1;
    rec[i] = v;
  }
  if (slot == 0 && tid < AS_HDR) {
    const int m = mem_len[u];
    const int limit = m < 1 ? 0 : min(min(m, pe_rows - 1), step_cap);
    int32_t v = 0;
    if (tid == AS_LIMIT) v = limit;
    if (tid == AS_DONE) v = limit < 1;                 // no memory frame: nothing to attend over, the utterance never starts
    if (tid == AS_MEM_ROW0) v = mem_row0[u];
    if (tid == AS_MEM_LEN) v = m;
    const_cast<int32_t*>(as_header(state, u))[tid] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- embed
// one work-group per row: x[r] = emb[last token] * sqrt(D) + pe[step]
__global__ __launch_bounds__(128) void aed_search_embed_kernel(const int32_t* __restrict__ state, int B, int N, int P, int rec_words,
                                                               const float* __restrict__ emb, const float* __restrict__ pe,
                                                               int pe_rows, int V, int D, float sqrt_d, float* __restrict__ x, int ldx) {
  const int r = blockIdx.x, u = r / N;
  const int32_t* hdr = as_header(state, u);
  const int s = hdr[AS_STEP];
  if (hdr[AS_DONE] != 0 || s < 0 || s >= P - 1 || s >= pe_rows) return;        // a done utterance keeps its stale row
  const int tok = as_record(state, B, rec_words, r, s & 1)[AS_TOKENS + s];
  const bool ok = tok >= 0 && tok < V;
  float* xr = x + (size_t)r * ldx;
  for (int c = threadIdx.x; c < (D >> 2); c += blockDim.x) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};                                            // a token outside [0, V) cannot arise; stay finite
    if (ok) {
      const f32x4 e = ldg4(emb + (size_t)tok * D + 4 * c), p = ldg4(pe + (size_t)s * D + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = e[j] * sqrt_d + p[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[4 * c + j] = o[j];
  }
}

// ------------------------------------------------------------------------------------------------------------ attention
// one wave per (row, head), four per work-group.  The query sits in LDS (read as a broadcast); lane j of a tile scores key j
// with 16-byte loads along its key row; the tile's maximum and sum go through the wave (online softmax); lane d accumulates
// output dimension d (and d + 64) with the probabilities and key rows broadcast from their lanes.  A key is (row index,
// own): own = the row's new K | V in `kv` (self use, position `step`), otherwise row `index` of the cache layer (self use)
// or of `kv` (source use: the memory rows of the row's utterance).  V lies D floats behind K in all three.
template <int DK>
__global__ __launch_bounds__(256) void aed_search_attention_kernel(const int32_t* __restrict__ state, int B, int N, int P, int rec_words,
                                                                   int H, int self, const float* __restrict__ q, int ldq,
                                                                   const float* __restrict__ kv, int ldkv, int kv_rows,
                                                                   float* __restrict__ cache, float scale, float* __restrict__ out,
                                                                   int ldo) {
  constexpr int DPL = (DK + 63) / 64;
  __shared__ float qs[4][DK];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int R = B * N, D = H * DK;
  const int pair = blockIdx.x * 4 + w;
  bool valid = pair < R * H;
  const int r = valid ? pair / H : 0, head = valid ? pair - r * H : 0;
  const int u = r / N;
  const int32_t* hdr = as_header(state, u);
  const int s = hdr[AS_STEP];
  valid = valid && hdr[AS_DONE] == 0 && s >= 0 && s < P - 1;     // rows of a done utterance are skipped: nothing is stored
  int n_keys = s + 1, mem_row0 = 0;
  if (!self) {
    mem_row0 = hdr[AS_MEM_ROW0];
    n_keys = hdr[AS_MEM_LEN];
    valid = valid && mem_row0 >= 0 && n_keys >= 1 && n_keys <= kv_rows - mem_row0;
  }
  const size_t col0 = (size_t)head * DK;
  if (valid)
    for (int c = lane; c < DK; c += 64) qs[w][c] = q[(size_t)r * ldq + col0 + c];
  __syncthreads();
  if (!valid) return;

  const float* own = kv + (size_t)r * ldkv + col0;               // self use: this row's new key, its value D floats behind
  if (self) {
    float* dst = cache + ((size_t)s * R + r) * 2 * D + col0;
    for (int c = lane; c < DK; c += 64) {
      dst[c] = own[c];
      dst[D + c] = own[D + c];
    }
  }
  const int32_t* path = as_record(state, B, rec_words, r, s & 1) + AS_TOKENS + P;

  float m = -INFINITY, l = 0.f, o[DPL];
#pragma unroll
  for (int c = 0; c < DPL; ++c) o[c] = 0.f;

  for (int t0 = 0; t0 < n_keys; t0 += 64) {
    const int t = t0 + lane;
    const bool vis = t < n_keys;
    int row = r, is_own = 1;
    if (self) {
      if (vis && t < s) {
        row = t * R + u * N + min(max(path[t], 0), N - 1);
        is_own = 0;
      }
    } else {
      row = mem_row0 + (vis ? t : 0);
      is_own = 0;
    }
    const float* kp = is_own ? own : (self ? cache + (size_t)row * 2 * D + col0 : kv + (size_t)row * ldkv + col0);
    float sc = 0.f;
    if (vis) {
#pragma unroll 4
      for (int e = 0; e < DK; e += 4) {
        const f32x4 kk = ldg4(kp + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) sc = fmaf(qs[w][e + j], kk[j], sc);
      }
    }
    sc = vis ? sc * scale : -INFINITY;
    const float m_new = fmaxf(m, wave_max(sc));                  // lane 0 of tile 0 is always visible: m_new is finite or NaN
    const float alpha = expf(m - m_new);                         // 0 for the first tile
    const float p = vis ? expf(sc - m_new) : 0.f;
    l = l * alpha + wave_sum(p);
    m = m_new;
#pragma unroll
    for (int c = 0; c < DPL; ++c) o[c] *= alpha;
    const int cnt = min(64, n_keys - t0);
    for (int j = 0; j < cnt; ++j) {
      const float pj = lane_bcast_f(p, j);
      const int row_j = lane_bcast_i(row, j), own_j = lane_bcast_i(is_own, j);
      const float* vp = (own_j ? own : (self ? cache + (size_t)row_j * 2 * D + col0 : kv + (size_t)row_j * ldkv + col0)) + D;
#pragma unroll
      for (int c = 0; c < DPL; ++c)
        if (lane + 64 * c < DK) o[c] = fmaf(pj, vp[lane + 64 * c], o[c]);
    }
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  float* orow = out + (size_t)r * ldo + col0;
#pragma unroll
  for (int c = 0; c < DPL; ++c)
    if (lane + 64 * c < DK) orow[lane + 64 * c] = o[c] * inv;
}

template <int DK>
static int launch_search_attention(const m3_aed_search_desc* d, const int32_t* state, int self, const float* q, int ldq,
                                   const float* kv, int ldkv, int kv_rows, float* cache, float* out, int ldo, hipStream_t stream) {
  const SearchLayout l = search_layout(d);
  const int pairs = d->B * d->beam * d->H;
  hipLaunchKernelGGL(aed_search_attention_kernel<DK>, dim3((unsigned)cdiv(pairs, 4)), dim3(256), 0, stream, state, d->B, d->beam, l.P,
                     l.rec_words, d->H, self, q, ldq, kv, ldkv, kv_rows, cache, 1.f / sqrtf((float)DK), out, ldo);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- prune
// (better_of / wave_best / wave_next_best, the pick order, are in aed_search_state.h)
// one work-group per utterance.  Wave w takes rows w, w + 4, ..: logsumexp over V and the N largest logits, or the single eos
// candidate of a finished slot; wave 0 then picks the N largest of the N * N candidates; all threads copy the parents' token
// and ancestry paths into the other record; thread 0 moves the step and decides whether the utterance is done.
__global__ __launch_bounds__(256) void aed_search_prune_kernel(int32_t* state, int B, int N, int P, int rec_words, int V,
                                                               const float* __restrict__ logits, int ldl,
                                                               int32_t* __restrict__ done_out) {
  __shared__ float c_score[AS_MAX_BEAM * AS_MAX_BEAM];
  __shared__ int32_t c_tok[AS_MAX_BEAM * AS_MAX_BEAM];
  __shared__ int32_t pick[AS_MAX_BEAM];
  const int u = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int32_t* hdr = as_header(state, u);
  const int s = hdr[AS_STEP], limit = hdr[AS_LIMIT];
  if (hdr[AS_DONE] != 0 || s < 0 || s >= P - 1) {                  // frozen: not one word of the utterance changes
    if (tid == 0 && done_out) done_out[u] = 1;
    return;
  }
  const int cur = s & 1, eos = V - 1;
  for (int i = w; i < N; i += 4) {
    const int row = u * N + i;
    const int32_t* rec = as_record(state, B, rec_words, row, cur);
    const float score = __builtin_bit_cast(float, rec[AS_SCORE]);
    if (rec[AS_FINISHED] != 0) {                                  // mask_finished_scores / _preds: increment 0, token eos
      if (lane < N) {
        c_score[i * N + lane] = lane == 0 ? score : -INFINITY;
        c_tok[i * N + lane] = eos;
      }
      continue;
    }
    const float* x = logits + (size_t)row * ldl;
    float mx = -INFINITY;
    for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < V; c += 64) sum += expf(x[c] - mx);
    const float lse = logf(wave_sum(sum));
    float pv = 0.f;
    int pi = -1;
    for (int k = 0; k < N; ++k) {
      float bv;
      int bi;
      wave_next_best(x, V, k == 0, pv, pi, lane, bv, bi);
      if (lane == 0) {
        c_score[i * N + k] = bi >= 0 ? score + ((bv - mx) - lse) : -INFINITY;   // -inf + increment stays -inf
        c_tok[i * N + k] = bi >= 0 ? bi : eos;
      }
      pv = bv;
      pi = bi;
      if (bi < 0) pv = -INFINITY, pi = INT_MAX;                   // nothing left (NaN logits): the rest of the row is -inf
    }
  }
  __syncthreads();
  if (w == 0) {
    float pv = 0.f;
    int pi = -1;
    for (int j = 0; j < N; ++j) {
      float bv;
      int bi;
      wave_next_best(c_score, N * N, j == 0, pv, pi, lane, bv, bi);
      if (lane == 0) pick[j] = bi;
      pv = bv;
      pi = bi;
      if (bi < 0) pv = -INFINITY, pi = INT_MAX;
    }
  }
  __syncthreads();
  const int nxt = cur ^ 1, span = s + 1;
  for (int idx = tid; idx < N * span; idx += 256) {
    const int j = idx / span, t = idx - j * span;
    const int parent = pick[j] >= 0 ? pick[j] / N : 0;
    const int32_t* src = as_record(state, B, rec_words, u * N + parent, cur);
    int32_t* dst = const_cast<int32_t*>(as_record(state, B, rec_words, u * N + j, nxt));
    dst[AS_TOKENS + t] = src[AS_TOKENS + t];
    dst[AS_TOKENS + P + t] = t < s ? src[AS_TOKENS + P + t] : parent;
  }
  if (tid < N) {
    const int j = tid, c = pick[j];
    const int tok = c >= 0 ? c_tok[c] : eos;
    int32_t* dst = const_cast<int32_t*>(as_record(state, B, rec_words, u * N + j, nxt));
    dst[AS_SCORE] = __builtin_bit_cast(int32_t, c >= 0 ? c_score[c] : -INFINITY);
    dst[AS_FINISHED] = tok == eos;
    dst[AS_TOKENS + s + 1] = tok;
  }
  if (tid == 0) {
    bool all = true;
    for (int j = 0; j < N; ++j) all = all && (pick[j] < 0 || c_tok[pick[j]] == eos);
    const int done = all || s + 1 >= limit;
    int32_t* h = const_cast<int32_t*>(hdr);
    h[AS_STEP] = s + 1;                                           // every thread read the header before the first barrier
    h[AS_DONE] = done;
    if (done_out) done_out[u] = done;
  }
}

// --------------------------------------------------------------------------------------------------------------- result
// one work-group (one wave) per utterance, lane j = slot j
__global__ __launch_bounds__(64) void aed_search_result_kernel(const int32_t* __restrict__ state, int B, int N, int P, int rec_words,
                                                               int V, int32_t* __restrict__ hyp_tokens, int32_t* __restrict__ hyp_len,
                                                               float* __restrict__ score, int32_t* __restrict__ finished,
                                                               int32_t* __restrict__ best, int32_t* __restrict__ steps) {
  __shared__ float sc[AS_MAX_BEAM];
  const int u = blockIdx.x, j = threadIdx.x, eos = V - 1, max_steps = P - 1;
  const int s = min(max(as_header(state, u)[AS_STEP], 0), max_steps);
  if (j < N) {
    const int row = u * N + j;
    const int32_t* rec = as_record(state, B, rec_words, row, s & 1);
    int n = s;
    while (n > 0 && rec[AS_TOKENS + n] == eos) --n;               // eos ends a hypothesis: all of them trail
    int32_t* y = hyp_tokens + (size_t)row * max_steps;
    for (int t = 0; t < max_steps; ++t) y[t] = t < n ? rec[AS_TOKENS + 1 + t] : -1;
    hyp_len[row] = n;
    sc[j] = __builtin_bit_cast(float, rec[AS_SCORE]);
    score[row] = sc[j];
    finished[row] = rec[AS_FINISHED];
  }
  __syncthreads();
  if (j == 0) {
    int arg = 0;
    for (int i = 1; i < N; ++i)
      if (sc[i] > sc[arg]) arg = i;                               // the first strictly largest
    best[u] = arg;
    steps[u] = s;
  }
}

}  // namespace
}  // namespace m3

using namespace m3;

extern "C" {

size_t m3_aed_search_state_size(const m3_aed_search_desc* desc) {
  if (check_search_desc(desc)) return 0;
  return search_state_bytes(desc);
}

size_t m3_aed_search_cache_size(const m3_aed_search_desc* desc) {
  if (check_search_desc(desc)) return 0;
  return search_cache_bytes(desc);
}

int m3_aed_search_reset(const m3_aed_search_desc* desc, void* state, size_t state_bytes, const int32_t* mem_row0,
                        const int32_t* mem_len, int max_steps, m3_stream stream) {
  if (int rc = check_search_state(desc, state, state_bytes, "aed_search_reset")) return rc;
  M3_REQUIRE(max_steps >= 1 && max_steps <= desc->max_steps, "aed_search_reset: max_steps = %d outside [1, %d]", max_steps, desc->max_steps);
  if (desc->B == 0) return 0;
  M3_REQUIRE(mem_row0 && mem_len, "aed_search_reset: null pointer");
  const SearchLayout l = search_layout(desc);
  hipLaunchKernelGGL(aed_search_reset_kernel, dim3((unsigned)(desc->B * desc->beam)), dim3(64), 0, (hipStream_t)stream, (int32_t*)state,
                     desc->B, desc->beam, l.rec_words, desc->V, desc->pe_rows, max_steps, mem_row0, mem_len);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_search_embed(const m3_aed_search_desc* desc, const void* state, size_t state_bytes, const float* emb, const float* pe,
                        float* x, int ldx, m3_stream stream) {
  if (int rc = check_search_state(desc, state, state_bytes, "aed_search_embed")) return rc;
  M3_REQUIRE((desc->D & 3) == 0 && ldx >= desc->D, "aed_search_embed: D = %d (a multiple of 4), ldx = %d", desc->D, ldx);
  if (desc->B == 0) return 0;
  M3_REQUIRE(emb && pe && x, "aed_search_embed: null pointer");
  M3_REQUIRE((((uintptr_t)emb | (uintptr_t)pe) & 15) == 0, "aed_search_embed: emb / pe must be 16-byte aligned");
  const SearchLayout l = search_layout(desc);
  hipLaunchKernelGGL(aed_search_embed_kernel, dim3((unsigned)(desc->B * desc->beam)), dim3(128), 0, (hipStream_t)stream,
                     (const int32_t*)state, desc->B, desc->beam, l.P, l.rec_words, emb, pe, desc->pe_rows, desc->V, desc->D,
                     sqrtf((float)desc->D), x, ldx);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_search_attention(const m3_aed_search_desc* desc, const void* state, size_t state_bytes, const float* q, int ldq,
                            const float* kv, int ldkv, int kv_rows, float* cache, size_t cache_bytes, int layer, float* out, int ldo,
                            m3_stream stream) {
  if (int rc = check_search_state(desc, state, state_bytes, "aed_search_attention")) return rc;
  const int D = desc->D, R = desc->B * desc->beam;
  M3_REQUIRE(ldq >= D && ldo >= D && ldkv >= 2 * D && (ldkv & 3) == 0, "aed_search_attention: ldq=%d, ldo=%d >= D = %d; ldkv=%d a multiple of 4 >= 2 D",
             ldq, ldo, D, ldkv);
  M3_REQUIRE(layer >= 0 && layer < desc->layers, "aed_search_attention: layer = %d outside [0, %d)", layer, desc->layers);
  if (desc->B == 0) return 0;
  M3_REQUIRE(q && kv && out, "aed_search_attention: null pointer");
  M3_REQUIRE(((uintptr_t)kv & 15) == 0, "aed_search_attention: kv must be 16-byte aligned");
  float* layer_cache = nullptr;
  if (cache) {                                                    // self use: kv = the R rows' new K | V
    M3_REQUIRE(((uintptr_t)cache & 15) == 0 && cache_bytes >= search_cache_bytes(desc), "aed_search_attention: cache %zu bytes < required %zu (16-byte aligned)",
               cache_bytes, search_cache_bytes(desc));
    M3_REQUIRE(kv_rows >= R, "aed_search_attention: kv_rows = %d < %d hypothesis rows", kv_rows, R);
    layer_cache = cache + (size_t)layer * desc->max_steps * R * 2 * D;
  } else {
    M3_REQUIRE(kv_rows >= 1, "aed_search_attention: no memory rows (kv_len = 0 is rejected: every query needs a visible key)");
  }
  const int self = cache != nullptr;
  hipStream_t s = (hipStream_t)stream;
#define M3_AED_SEARCH_ATT(DK) \
  case DK: return launch_search_attention<DK>(desc, (const int32_t*)state, self, q, ldq, kv, ldkv, kv_rows, layer_cache, out, ldo, s)
  switch (D / desc->H) {
    M3_AED_SEARCH_ATT(16);
    M3_AED_SEARCH_ATT(32);
    M3_AED_SEARCH_ATT(48);
    M3_AED_SEARCH_ATT(64);
    M3_AED_SEARCH_ATT(80);
    M3_AED_SEARCH_ATT(96);
    M3_AED_SEARCH_ATT(112);
    M3_AED_SEARCH_ATT(128);
  }
#undef M3_AED_SEARCH_ATT
  m3::set_error("aed_search_attention: dk=%d", D / desc->H);
  return -2;
}

int m3_aed_search_prune(const m3_aed_search_desc* desc, void* state, size_t state_bytes, const float* logits, int ldl,
                        int32_t* done, m3_stream stream) {
  if (int rc = check_search_state(desc, state, state_bytes, "aed_search_prune")) return rc;
  M3_REQUIRE(ldl >= desc->V, "aed_search_prune: ldl = %d < V = %d", ldl, desc->V);
  if (desc->B == 0) return 0;
  M3_REQUIRE(logits != nullptr, "aed_search_prune: null pointer");
  const SearchLayout l = search_layout(desc);
  hipLaunchKernelGGL(aed_search_prune_kernel, dim3((unsigned)desc->B), dim3(256), 0, (hipStream_t)stream, (int32_t*)state, desc->B,
                     desc->beam, l.P, l.rec_words, desc->V, logits, ldl, done);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_search_result(const m3_aed_search_desc* desc, const void* state, size_t state_bytes, int32_t* hyp_tokens, int32_t* hyp_len,
                         float* score, int32_t* finished, int32_t* best, int32_t* steps, m3_stream stream) {
  if (int rc = check_search_state(desc, state, state_bytes, "aed_search_result")) return rc;
  if (desc->B == 0) return 0;
  M3_REQUIRE(hyp_tokens && hyp_len && score && finished && best && steps, "aed_search_result: null pointer");
  const SearchLayout l = search_layout(desc);
  hipLaunchKernelGGL(aed_search_result_kernel, dim3((unsigned)desc->B), dim3(64), 0, (hipStream_t)stream, (const int32_t*)state, desc->B,
                     desc->beam, l.P, l.rec_words, desc->V, hyp_tokens, hyp_len, score, finished, best, steps);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
