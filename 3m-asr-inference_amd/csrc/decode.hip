// what sits after the encoder (CTC search on the logits) and the reference's streaming operators.
//
//  * CTC greedy search (trainer_3m_fix/model/encoder.py:156-180): per frame argmax over the vocabulary, then per
//    utterance "drop repeats, drop blank" over the frames t < len[b].  The reference does the argmax on the device and the
//    collapse in a Python loop on the host; here both are kernels (one wave per frame, one wave per utterance with a
//    ballot / prefix-popcount compaction), so the result that leaves the GPU is the token list, not (B,T',V) scores.
//  * CTC prefix beam search (encoder.py:182-275): the per-frame log-softmax and first beam prune (`logp.topk(beam)`,
//    :224-231) run on the device -- only T'*k (value, index) pairs cross to the host instead of T'*V scores -- and the
//    sequential prefix recursion (:232-273) is a host routine over those pairs, in double precision like the Python floats
//    of the reference.
//  * The streaming operators of the plugin library (registration commented out in trt_plugin_plus.cpp:155-156; no model in
//    the tree uses them): CatSplitCache (cat_split_cache_kernel.cu:30-107), AttStreamSoftmax
//    (att_stream_softmax_kernel.cu:28-191) and RelPositionalEncoding with a frame offset
//    (rel_positional_encoding_kernel.cu:62-69,108-123).
#include <algorithm>
#include <cfloat>
#include <limits>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace m3 {

// ---------------------------------------------------------------- CTC greedy search
// (value, index) argmax with "first maximum wins" (torch.argmax): lexicographic (value desc, index asc)
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    argmax_merge(v, i, ov, oi);
  }
}

// one wave per frame: ids[row] = argmax_j logits[row][j]
__global__ __launch_bounds__(256) void ctc_argmax_kernel(const float* __restrict__ logits, size_t rows, int V,
                                                         int32_t* __restrict__ ids) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const float* xr = logits + row * V;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int j = lane; j < V; j += 64) {
    const float v = xr[j];
    if (v > best || bi == 0x7fffffff) {   // ascending j: a later equal value never replaces an earlier one
      best = v;
      bi = j;
    }
  }
  wave_argmax(best, bi);
  if (lane == 0) ids[row] = bi;
}

// one wave per utterance: keep frame t iff t < len, ids[t] != blank and ids[t] != ids[t-1]; stable compaction
__global__ __launch_bounds__(64) void ctc_collapse_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ len,
                                                          int T, int blank, int32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ n_tokens) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = len ? min(max(len[b], 0), T) : T;
  const int32_t* row = ids + (size_t)b * T;
  int32_t* out = tokens + (size_t)b * T;
  int count = 0;
  for (int t0 = 0; t0 < n; t0 += 64) {
    const int t = t0 + lane;
    bool keep = false;
    int id = blank;
    if (t < n) {
      id = row[t];
      keep = id != blank && (t == 0 || id != row[t - 1]);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) out[count + __popcll(m & ((1ull << lane) - 1ull))] = id;
    count += __popcll(m);
  }
  for (int t = count + lane; t < T; t += 64) out[t] = -1;
  if (lane == 0) n_tokens[b] = count;
}

int launch_ctc_greedy(const float* logits, const int32_t* len, int B, int T, int V, int blank, int32_t* frame_ids,
                      int32_t* tokens, int32_t* n_tokens, hipStream_t stream) {
  M3_REQUIRE(B >= 0 && T >= 0 && V > 0, "ctc_greedy: bad shape B=%d T=%d V=%d", B, T, V);
  if (B == 0) return 0;
  const size_t rows = (size_t)B * T;
  if (rows)
    hipLaunchKernelGGL(ctc_argmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, logits, rows, V, frame_ids);
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(64), 0, stream, frame_ids, len, T, blank, tokens, n_tokens);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_ctc_argmax(const float* logits, size_t rows, int V, int32_t* ids, hipStream_t stream) {
  M3_REQUIRE(V > 0, "ctc_argmax: V = %d", V);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ctc_argmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, logits, rows, V, ids);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- per-frame log-softmax + top-k (first beam prune)
// One wave per frame.  Selection order is (value desc, index asc); round r picks the best element strictly after the
// previous pick in that order, so nothing is mutated and the row is only re-read (from L1/L2) k times.
__global__ __launch_bounds__(256) void ctc_topk_kernel(const float* __restrict__ logits, size_t rows, int V, int k,
                                                       float* __restrict__ top_logp, int32_t* __restrict__ top_idx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const float* xr = logits + row * V;
  float mx = -INFINITY;
  for (int j = lane; j < V; j += 64) mx = fmaxf(mx, xr[j]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < V; j += 64) sum += expf(xr[j] - mx);
  const float lse = mx + logf(wave_sum(sum));
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < k; ++r) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = lane; j < V; j += 64) {
      const float v = xr[j];
      const bool after = v < pv || (v == pv && j > pi);
      if (after && (bi == 0x7fffffff || v > best)) {
        best = v;
        bi = j;
      }
    }
    wave_argmax(best, bi);
    if (lane == 0) {
      top_logp[row * k + r] = best - lse;
      top_idx[row * k + r] = bi;
    }
    pv = best;
    pi = bi;
  }
}

int launch_ctc_topk(const float* logits, size_t rows, int V, int k, float* top_logp, int32_t* top_idx, hipStream_t stream) {
  M3_REQUIRE(V > 0 && k > 0 && k <= V, "ctc_topk: need 0 < k <= V (k=%d, V=%d)", k, V);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ctc_topk_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, logits, rows, V, k, top_logp,
                     top_idx);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- CTC prefix beam search, host side
namespace {
const double NEG_INF = -std::numeric_limits<double>::infinity();
// utils/common.py:148-156, for up to three terms
inline double log_add3(double a, double b, double c) {
  if (a == NEG_INF && b == NEG_INF && c == NEG_INF) return NEG_INF;
  const double m = std::max(a, std::max(b, c));
  return m + std::log(std::exp(a - m) + std::exp(b - m) + std::exp(c - m));
}
inline double log_add2(double a, double b) {
  if (a == NEG_INF && b == NEG_INF) return NEG_INF;
  const double m = std::max(a, b);
  return m + std::log(std::exp(a - m) + std::exp(b - m));
}
struct Hyp {
  std::vector<int32_t> prefix;
  double pb, pnb;   // log prob of the prefix ending in blank / in a non-blank
};
}  // namespace

int ctc_prefix_beam_search_host(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, int32_t* n_hyps) {
  M3_REQUIRE(T >= 0 && k > 0 && beam > 0, "ctc_prefix_beam_search: bad sizes T=%d k=%d beam=%d", T, k, beam);
  M3_REQUIRE(top_logp && top_idx && hyp_tokens && hyp_len && hyp_score && n_hyps, "ctc_prefix_beam_search: null pointer");
  std::vector<Hyp> cur(1);
  cur[0].pb = 0.0;
  cur[0].pnb = NEG_INF;
  std::vector<Hyp> next;
  std::map<std::vector<int32_t>, int> where;   // prefix -> slot in `next` (slots keep first-touch order, as a dict does)
  std::vector<int> order;
  std::vector<double> key;
  auto slot = [&](const std::vector<int32_t>& p) -> Hyp& {
    auto it = where.find(p);
    if (it == where.end()) {
      it = where.emplace(p, (int)next.size()).first;
      next.push_back(Hyp{p, NEG_INF, NEG_INF});
    }
    return next[it->second];
  };
  std::vector<int32_t> ext;
  for (int t = 0; t < T; ++t) {
    next.clear();
    where.clear();
    for (int j = 0; j < k; ++j) {
      const int32_t s = top_idx[(size_t)t * k + j];
      const double ps = (double)top_logp[(size_t)t * k + j];
      for (size_t h = 0; h < cur.size(); ++h) {
        // `cur` is not touched while `next` grows: copy what is needed before slot() may reallocate `next`
        const double pb = cur[h].pb, pnb = cur[h].pnb;
        const std::vector<int32_t>& prefix = cur[h].prefix;
        const bool has_last = !prefix.empty();
        if (s == blank) {
          Hyp& n = slot(prefix);
          n.pb = log_add3(n.pb, pb + ps, pnb + ps);
        } else if (has_last && s == prefix.back()) {
          {
            Hyp& n = slot(prefix);              // ...s s  -> ...s
            n.pnb = log_add2(n.pnb, pnb + ps);
          }
          ext = prefix;
          ext.push_back(s);
          Hyp& n = slot(ext);                   // ...s - s -> ...s s
          n.pnb = log_add2(n.pnb, pb + ps);
        } else {
          ext = prefix;
          ext.push_back(s);
          Hyp& n = slot(ext);
          n.pnb = log_add3(n.pnb, pb + ps, pnb + ps);
        }
      }
    }
    // second prune: best `beam` by total score, ties in first-touch order (Python's sorted(reverse=True) is stable)
    order.resize(next.size());
    key.resize(next.size());
    for (size_t i = 0; i < next.size(); ++i) {
      order[i] = (int)i;
      key[i] = log_add2(next[i].pb, next[i].pnb);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] > key[b]; });
    const size_t keep = std::min(order.size(), (size_t)beam);
    std::vector<Hyp> pruned;
    pruned.reserve(keep);
    for (size_t i = 0; i < keep; ++i) pruned.push_back(std::move(next[order[i]]));
    cur.swap(pruned);
  }
  const int n = (int)std::min(cur.size(), (size_t)beam);
  for (int i = 0; i < n; ++i) {
    const int L = (int)cur[i].prefix.size();
    hyp_len[i] = L;
    for (int j = 0; j < L; ++j) hyp_tokens[(size_t)i * T + j] = cur[i].prefix[j];
    for (int j = L; j < T; ++j) hyp_tokens[(size_t)i * T + j] = -1;
    hyp_score[i] = (float)log_add2(cur[i].pb, cur[i].pnb);
  }
  *n_hyps = n;
  return 0;
}

// ---------------------------------------------------------------- context biasing, host side
// Structure of a context image (kernels.h): the header, every graph's tables inside the image, and every table entry that
// the searches use as an index.  The limits: G <= 1024, n_states <= 65536, A <= min(V + 1, 65536), image <= 64 MiB.
int ctc_context_validate(const void* image, size_t bytes, int V) {
  M3_REQUIRE(image != nullptr, "ctc_context_validate: null image");
  M3_REQUIRE(V >= 1, "ctc_context_validate: V = %d < 1", V);
  M3_REQUIRE(bytes % 4 == 0 && bytes >= CTX_HDR_WORDS * 4 && bytes <= kCtxMaxBytes,
             "ctc_context_validate: image of %zu bytes (a multiple of 4 in [%d, %zu])", bytes, CTX_HDR_WORDS * 4, kCtxMaxBytes);
  const int32_t* w = (const int32_t*)image;
  const long long words = (long long)(bytes / 4);
  M3_REQUIRE(w[CTX_MAGIC] == kCtxMagic, "ctc_context_validate: not a context image");
  M3_REQUIRE(w[CTX_V] == V, "ctc_context_validate: image built for V = %d, asked for V = %d", w[CTX_V], V);
  M3_REQUIRE(w[CTX_WORDS] == words, "ctc_context_validate: image says %d words, has %lld", w[CTX_WORDS], words);
  const int G = w[CTX_G];
  M3_REQUIRE(G >= 0 && G <= kCtxMaxGraphs && CTX_HDR_WORDS + (long long)G * CTXG_WORDS <= words,
             "ctc_context_validate: G = %d outside [0, %d] or its headers outside the image", G, kCtxMaxGraphs);
  for (int g = 0; g < G; ++g) {
    CtxGraph c;
    M3_REQUIRE(ctx_graph_view(w, words, g, &c),
               "ctc_context_validate: graph %d: n_states outside [1, %d], A outside [1, min(V + 1, %d)] or a table outside the image",
               g, kCtxMaxStates, kCtxMaxStates);
    for (int v = 0; v < V; ++v)
      M3_REQUIRE(c.cls[v] >= 0 && c.cls[v] < c.A, "ctc_context_validate: graph %d: cls[%d] = %d outside [0, %d)", g, v, c.cls[v], c.A);
    for (long long i = 0; i < (long long)c.n_states * c.A; ++i) {
      M3_REQUIRE(c.next[i] >= 0 && c.next[i] < c.n_states, "ctc_context_validate: graph %d: next[%lld] = %d outside [0, %d)", g, i,
                 c.next[i], c.n_states);
      M3_REQUIRE(std::isfinite(c.delta[i]), "ctc_context_validate: graph %d: delta[%lld] is not finite", g, i);
    }
    for (int s = 0; s < c.n_states; ++s)
      M3_REQUIRE(std::isfinite(c.pot[s]), "ctc_context_validate: graph %d: pot[%d] is not finite", g, s);
  }
  return 0;
}

// ---------------------------------------------------------------- n-gram LM shallow fusion, host side
// Structure of an LM image (kernels.h): the header and limits, every table inside the image, and every table entry that the
// searches use as an index or add to a score.  Limits: order <= 8, n_states <= 2^26, image <= 1 GiB.
static int ctc_lm_set_validate(const int32_t* w, size_t bytes, int V);
int ctc_lm_validate(const void* image, size_t bytes, int V) {
  M3_REQUIRE(image != nullptr, "ctc_lm_validate: null image");
  M3_REQUIRE(V >= 1, "ctc_lm_validate: V = %d < 1", V);
  if (bytes % 4 == 0 && lm_is_set((const int32_t*)image, (long long)(bytes / 4))) return ctc_lm_set_validate((const int32_t*)image, bytes, V);
  M3_REQUIRE(bytes % 4 == 0 && bytes >= LM_HDR_WORDS * 4 && bytes <= kLmMaxBytes,
             "ctc_lm_validate: image of %zu bytes (a multiple of 4 in [%d, %zu])", bytes, LM_HDR_WORDS * 4, kLmMaxBytes);
  const int32_t* w = (const int32_t*)image;
  const long long words = (long long)(bytes / 4);
  M3_REQUIRE(w[LM_MAGIC] == kLmMagic, "ctc_lm_validate: not an LM image");
  M3_REQUIRE(w[LM_VERSION] == kLmVersion, "ctc_lm_validate: image version %d, this library reads version %d", w[LM_VERSION],
             kLmVersion);
  M3_REQUIRE(w[LM_V] == V, "ctc_lm_validate: image built for V = %d, asked for V = %d", w[LM_V], V);
  M3_REQUIRE(w[LM_WORDS] == words, "ctc_lm_validate: image says %d words, has %lld", w[LM_WORDS], words);
  LmView m;
  M3_REQUIRE(lm_view(w, words, &m),
             "ctc_lm_validate: order outside [1, %d], n_states outside [1, %d], n_arcs < 0, start outside [0, n_states) or a "
             "table outside the image", kLmMaxOrder, kLmMaxStates);
  M3_REQUIRE(std::isfinite(m.unk_logp), "ctc_lm_validate: unk_logp is not finite");
  for (int v = 0; v < V; ++v) {
    M3_REQUIRE(std::isfinite(m.uni_logp[v]), "ctc_lm_validate: uni_logp[%d] is not finite", v);
    M3_REQUIRE(m.uni_next[v] >= 0 && m.uni_next[v] < m.n_states, "ctc_lm_validate: uni_next[%d] = %d outside [0, %d)", v,
               m.uni_next[v], m.n_states);
  }
  M3_REQUIRE(m.arc_begin[0] == 0 && m.arc_begin[1] == 0, "ctc_lm_validate: arc_begin[0..1] = %d, %d (state 0 has no sparse arcs)",
             m.arc_begin[0], m.arc_begin[1]);
  M3_REQUIRE(m.arc_begin[m.n_states] == m.n_arcs, "ctc_lm_validate: arc_begin[n_states] = %d, n_arcs = %d", m.arc_begin[m.n_states],
             m.n_arcs);
  std::vector<unsigned char> depth((size_t)m.n_states, 0);     // levels of the back-off chain above state 0
  for (int s = 0; s < m.n_states; ++s) {
    const int lo = m.arc_begin[s], hi = m.arc_begin[s + 1];
    M3_REQUIRE(lo >= 0 && lo <= hi && hi <= m.n_arcs, "ctc_lm_validate: arc_begin[%d..] = %d, %d is not monotone in [0, %d]", s, lo,
               hi, m.n_arcs);
    for (int i = lo; i < hi; ++i) {
      M3_REQUIRE(m.arc_tok[i] >= 0 && m.arc_tok[i] < V, "ctc_lm_validate: arc_tok[%d] = %d outside [0, %d)", i, m.arc_tok[i], V);
      M3_REQUIRE(i == lo || m.arc_tok[i - 1] < m.arc_tok[i], "ctc_lm_validate: arc_tok[%d] = %d is not above arc_tok[%d] = %d (state %d)",
                 i, m.arc_tok[i], i - 1, m.arc_tok[i - 1], s);
      M3_REQUIRE(m.arc_next[i] >= 0 && m.arc_next[i] < m.n_states, "ctc_lm_validate: arc_next[%d] = %d outside [0, %d)", i,
                 m.arc_next[i], m.n_states);
      M3_REQUIRE(std::isfinite(m.arc_logp[i]), "ctc_lm_validate: arc_logp[%d] is not finite", i);
    }
    M3_REQUIRE(s == 0 ? m.bo_state[0] == 0 : (m.bo_state[s] >= 0 && m.bo_state[s] < s),
               "ctc_lm_validate: bo_state[%d] = %d (0 for state 0, else in [0, %d))", s, m.bo_state[s], s);
    if (s > 0) {
      depth[s] = (unsigned char)(depth[m.bo_state[s]] + 1);
      M3_REQUIRE(depth[s] < m.order, "ctc_lm_validate: back-off chain of state %d has %d levels, order %d", s, (int)depth[s],
                 m.order);
    }
    M3_REQUIRE(std::isfinite(m.bo_weight[s]), "ctc_lm_validate: bo_weight[%d] is not finite", s);
    M3_REQUIRE(std::isfinite(m.fin[s]), "ctc_lm_validate: final[%d] is not finite", s);
  }
  return 0;
}

// Structure of an LM set (kernels.h): the header, the directory -- every member 16-byte aligned, behind the directory, in
// ascending order without overlap, inside the set, its scale finite and positive -- and every member by the rules above.
static int ctc_lm_set_validate(const int32_t* w, size_t bytes, int V) {
  const long long words = (long long)(bytes / 4);
  M3_REQUIRE(bytes <= kLmSetMaxBytes, "ctc_lm_validate: LM set of %zu bytes > %zu", bytes, kLmSetMaxBytes);
  M3_REQUIRE(w[LMS_VERSION] == kLmSetVersion, "ctc_lm_validate: LM set version %d, this library reads version %d", w[LMS_VERSION],
             kLmSetVersion);
  M3_REQUIRE(w[LMS_V] == V, "ctc_lm_validate: LM set built for V = %d, asked for V = %d", w[LMS_V], V);
  const int G = w[LMS_G];
  M3_REQUIRE(G >= 1 && G <= kLmSetMaxMembers, "ctc_lm_validate: LM set with G = %d members outside [1, %d]", G, kLmSetMaxMembers);
  M3_REQUIRE(w[LMS_WORDS] == words, "ctc_lm_validate: LM set says %d words, has %lld", w[LMS_WORDS], words);
  M3_REQUIRE(w[5] == 0 && w[6] == 0 && w[7] == 0, "ctc_lm_validate: LM set header words 5..7 are not 0");
  long long end = LMS_HDR_WORDS + (long long)G * LMS_ENTRY_WORDS;            // the first word a member may take
  M3_REQUIRE(end <= words, "ctc_lm_validate: LM set of %lld words cannot hold a directory of %d entries", words, G);
  for (int j = 0; j < G; ++j) {
    const int32_t* e = w + LMS_HDR_WORDS + (size_t)j * LMS_ENTRY_WORDS;
    const long long off = e[LMS_E_OFFSET], n = e[LMS_E_WORDS];
    const float scale = ((const float*)e)[LMS_E_SCALE];
    M3_REQUIRE(off >= 0 && off % 4 == 0, "ctc_lm_validate: LM set member %d: offset of %lld words is not a multiple of 4 (16-byte alignment)",
               j, off);
    M3_REQUIRE(off >= end, "ctc_lm_validate: LM set member %d at word %lld overlaps what ends at word %lld (the directory or member %d)",
               j, off, end, j - 1);
    M3_REQUIRE(n >= LM_HDR_WORDS && off <= words && n <= words - off,
               "ctc_lm_validate: LM set member %d: words [%lld, %lld) reach past the end of the set (%lld words) or hold no header", j, off,
               off + n, words);
    M3_REQUIRE(std::isfinite(scale) && scale > 0.f, "ctc_lm_validate: LM set member %d: scale = %g is not finite and positive", j,
               (double)scale);
    M3_REQUIRE(e[3] == 0, "ctc_lm_validate: LM set member %d: directory word 3 is not 0", j);
    M3_REQUIRE(w[off + LM_MAGIC] == kLmMagic, "ctc_lm_validate: LM set member %d is not an LM image", j);
    if (int rc = ctc_lm_validate(w + off, (size_t)n * 4, V)) {
      const std::string why = last_error();
      set_error("ctc_lm_validate: LM set member %d: %s", j, why.c_str());
      return rc;
    }
    end = off + n;
  }
  return 0;
}

// Member j of a host set that passes ctc_lm_validate (run here): where it lies, its bytes and its scale.
int ctc_lm_set_member(const void* image, size_t bytes, int j, const void** member, size_t* member_bytes, float* scale) {
  M3_REQUIRE(image != nullptr && member != nullptr && member_bytes != nullptr, "ctc_lm_set_member: null pointer");
  M3_REQUIRE(bytes % 4 == 0 && lm_is_set((const int32_t*)image, (long long)(bytes / 4)), "ctc_lm_set_member: not an LM set");
  const int32_t* w = (const int32_t*)image;
  if (int rc = ctc_lm_set_validate(w, bytes, w[LMS_V])) return rc;
  M3_REQUIRE(j >= 0 && j < w[LMS_G], "ctc_lm_set_member: member %d outside [0, %d)", j, w[LMS_G]);
  const int32_t* e = w + LMS_HDR_WORDS + (size_t)j * LMS_ENTRY_WORDS;
  *member = w + e[LMS_E_OFFSET];
  *member_bytes = (size_t)e[LMS_E_WORDS] * 4;
  if (scale) *scale = ((const float*)e)[LMS_E_SCALE];
  return 0;
}

// ctc_prefix_beam_search_host with the fused ranking.  Every prefix carries (state, bonus) of its walk through graph `graph`
// of the context image and (lm_state, lm) of its walk through the LM (lm = the left-to-right double sum of lm_step from the
// LM's start state).  The second prune ranks by (log_add2(pb, pnb) + bonus) + (alpha lm + beta |prefix|); the hypotheses come
// out ordered by (log_add2(pb, pnb) + final) + (alpha (lm + fin[lm_state] use_eos) + beta |prefix|), stable on the beam
// order (final = bonus - pot[state]).  Without a graph: state 0 and bonus 0.0 throughout, and x + 0.0 == x.  Without an LM
// the second bracket is not added at all: the biased routine's result, and without either the unbiased routine's.
int ctc_prefix_beam_search_lm_host(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                   const void* image, size_t image_bytes, int graph, const void* lm_image, size_t lm_bytes,
                                   double alpha, double beta, int use_eos, int32_t* hyp_tokens, int32_t* hyp_len,
                                   float* hyp_score, float* hyp_bonus, int32_t* hyp_state, float* hyp_lm, int32_t* n_hyps) {
  const char* who = lm_image ? "ctc_prefix_beam_search_lm" : "ctc_prefix_beam_search_ctx";
  M3_REQUIRE(T >= 0 && k > 0 && beam > 0, "%s: bad sizes T=%d k=%d beam=%d", who, T, k, beam);
  M3_REQUIRE(top_logp && top_idx && hyp_tokens && hyp_len && hyp_score && hyp_bonus && hyp_state && n_hyps, "%s: null pointer", who);
  CtxGraph g{};
  const bool biased = image != nullptr && graph != -1;
  if (biased) {
    M3_REQUIRE(image_bytes >= CTX_HDR_WORDS * 4, "%s: image of %zu bytes", who, image_bytes);
    if (int rc = ctc_context_validate(image, image_bytes, ((const int32_t*)image)[CTX_V])) return rc;
    M3_REQUIRE(ctx_graph_view((const int32_t*)image, (long long)(image_bytes / 4), graph, &g), "%s: graph %d is not in the image",
               who, graph);
  }
  LmView lm{};
  const bool fused = lm_image != nullptr;
  if (fused) {
    M3_REQUIRE(hyp_lm != nullptr, "%s: null hyp_lm", who);
    M3_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "%s: alpha or beta is not finite", who);
    M3_REQUIRE(lm_bytes >= LM_HDR_WORDS * 4, "%s: LM image of %zu bytes", who, lm_bytes);
    if (int rc = ctc_lm_validate(lm_image, lm_bytes, ((const int32_t*)lm_image)[LM_V])) return rc;
    lm_view((const int32_t*)lm_image, (long long)(lm_bytes / 4), &lm);
  }
  struct CHyp {
    std::vector<int32_t> prefix;
    double pb, pnb;
    int state;
    double bonus;
    int lm_state;
    double lm;
  };
  std::vector<CHyp> cur(1);
  cur[0].pb = 0.0;
  cur[0].pnb = NEG_INF;
  cur[0].state = 0;
  cur[0].bonus = 0.0;
  cur[0].lm_state = fused ? lm.start : 0;
  cur[0].lm = 0.0;
  std::vector<CHyp> next;
  std::map<std::vector<int32_t>, int> where;
  std::vector<int> order;
  std::vector<double> key;
  auto slot = [&](const std::vector<int32_t>& p, int state, double bonus, int lm_state, double lm_sum) -> CHyp& {
    auto it = where.find(p);
    if (it == where.end()) {
      it = where.emplace(p, (int)next.size()).first;
      next.push_back(CHyp{p, NEG_INF, NEG_INF, state, bonus, lm_state, lm_sum});
    }
    return next[it->second];
  };
  std::vector<int32_t> ext;
  for (int t = 0; t < T; ++t) {
    next.clear();
    where.clear();
    for (int j = 0; j < k; ++j) {
      const int32_t s = top_idx[(size_t)t * k + j];
      const double ps = (double)top_logp[(size_t)t * k + j];
      const int col = biased && s >= 0 && s < g.V ? g.cls[s] : 0;
      for (size_t h = 0; h < cur.size(); ++h) {
        const double pb = cur[h].pb, pnb = cur[h].pnb, bonus = cur[h].bonus, lm_sum = cur[h].lm;
        const int state = cur[h].state, lm_state = cur[h].lm_state;
        const std::vector<int32_t>& prefix = cur[h].prefix;
        const bool has_last = !prefix.empty();
        int e_state = 0, e_lm_state = 0;
        double e_bonus = bonus, e_lm = 0.0;
        if (biased) {
          e_state = g.next[(size_t)state * g.A + col];
          e_bonus = bonus + (double)g.delta[(size_t)state * g.A + col];
        }
        if (fused && s != blank) e_lm = lm_sum + lm_step(lm, lm_state, s, &e_lm_state);
        if (s == blank) {
          CHyp& n = slot(prefix, state, bonus, lm_state, lm_sum);
          n.pb = log_add3(n.pb, pb + ps, pnb + ps);
        } else if (has_last && s == prefix.back()) {
          {
            CHyp& n = slot(prefix, state, bonus, lm_state, lm_sum);
            n.pnb = log_add2(n.pnb, pnb + ps);
          }
          ext = prefix;
          ext.push_back(s);
          CHyp& n = slot(ext, e_state, e_bonus, e_lm_state, e_lm);
          n.pnb = log_add2(n.pnb, pb + ps);
        } else {
          ext = prefix;
          ext.push_back(s);
          CHyp& n = slot(ext, e_state, e_bonus, e_lm_state, e_lm);
          n.pnb = log_add3(n.pnb, pb + ps, pnb + ps);
        }
      }
    }
    order.resize(next.size());
    key.resize(next.size());
    for (size_t i = 0; i < next.size(); ++i) {
      order[i] = (int)i;
      key[i] = log_add2(next[i].pb, next[i].pnb) + next[i].bonus;
      if (fused) key[i] = key[i] + (alpha * next[i].lm + beta * (double)next[i].prefix.size());
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] > key[b]; });
    const size_t keep = std::min(order.size(), (size_t)beam);
    std::vector<CHyp> pruned;
    pruned.reserve(keep);
    for (size_t i = 0; i < keep; ++i) pruned.push_back(std::move(next[order[i]]));
    cur.swap(pruned);
  }
  const int n = (int)std::min(cur.size(), (size_t)beam);
  order.resize(n);
  key.resize(n);
  std::vector<double> fin(n), lmf(n, 0.0);
  for (int i = 0; i < n; ++i) {
    order[i] = i;
    fin[i] = cur[i].bonus - (biased ? (double)g.pot[cur[i].state] : 0.0);
    key[i] = log_add2(cur[i].pb, cur[i].pnb) + fin[i];
    if (fused) {
      lmf[i] = cur[i].lm + (use_eos ? (double)lm.fin[cur[i].lm_state] : 0.0);
      key[i] = key[i] + (alpha * lmf[i] + beta * (double)cur[i].prefix.size());
    }
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] > key[b]; });
  for (int r = 0; r < n; ++r) {
    const CHyp& hyp = cur[order[r]];
    const int L = (int)hyp.prefix.size();
    hyp_len[r] = L;
    for (int j = 0; j < L; ++j) hyp_tokens[(size_t)r * T + j] = hyp.prefix[j];
    for (int j = L; j < T; ++j) hyp_tokens[(size_t)r * T + j] = -1;
    hyp_score[r] = (float)log_add2(hyp.pb, hyp.pnb);
    hyp_bonus[r] = (float)fin[order[r]];
    hyp_state[r] = hyp.state;
    if (hyp_lm) hyp_lm[r] = (float)lmf[order[r]];
  }
  *n_hyps = n;
  return 0;
}

// the biased routine: the fused one without an LM
int ctc_prefix_beam_search_ctx_host(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                    const void* image, size_t image_bytes, int graph, int32_t* hyp_tokens, int32_t* hyp_len,
                                    float* hyp_score, float* hyp_bonus, int32_t* hyp_state, int32_t* n_hyps) {
  return ctc_prefix_beam_search_lm_host(top_logp, top_idx, T, k, beam, blank, image, image_bytes, graph, nullptr, 0, 0.0, 0.0, 0,
                                        hyp_tokens, hyp_len, hyp_score, hyp_bonus, hyp_state, nullptr, n_hyps);
}

// ---------------------------------------------------------------- CatSplitCache
// output[b] = in_cache[b] ++ input[b]  (cache_dim + input_dim values);  out_cache[b] = the last cache_dim values of
// output[b] (cat_split_cache_kernel.cu:30-107: both of the reference's branches, input_dim >= cache_dim and
// input_dim < cache_dim, compute exactly this).  One pass, 4-byte elements (f32 or i32 alike).
__global__ void cat_split_cache_kernel(const uint32_t* __restrict__ in_cache, const uint32_t* __restrict__ input, int cache_dim,
                                       int input_dim, uint32_t* __restrict__ output, uint32_t* __restrict__ out_cache,
                                       size_t n) {
  const int tot = cache_dim + input_dim;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / tot;
    const int o = (int)(i - b * tot);
    const uint32_t v = o < cache_dim ? in_cache[b * cache_dim + o] : input[b * input_dim + (o - cache_dim)];
    output[i] = v;
    if (o >= input_dim) out_cache[b * cache_dim + (o - input_dim)] = v;   // o >= tot - cache_dim
  }
}
int launch_cat_split_cache(const void* in_cache, const void* input, int B, int cache_dim, int input_dim, void* output,
                           void* out_cache, hipStream_t stream) {
  M3_REQUIRE(B >= 0 && cache_dim >= 0 && input_dim >= 0, "cat_split_cache: bad shape");
  M3_REQUIRE(out_cache != in_cache || cache_dim == 0, "cat_split_cache: out_cache must not alias in_cache");
  const size_t n = (size_t)B * (cache_dim + input_dim);
  if (n == 0) return 0;
  hipLaunchKernelGGL(cat_split_cache_kernel, dim3(grid1d(n, 2048)), dim3(256), 0, stream, (const uint32_t*)in_cache,
                     (const uint32_t*)input, cache_dim, input_dim, (uint32_t*)output, (uint32_t*)out_cache, n);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- AttStreamSoftmax
// scores [B][N][ld] (N = heads x query frames, ld = cache + chunk key positions).  Row (b, n) is valid on
// [first, last): first = max(0, ld - decode_frame_num[b]), last = min(ld, mask_idx[b]) + cache_len, and
//   out[j] = exp((x[j] - max_valid x) * scale) / sum_valid exp((x - max) * scale),   0 outside [first, last)
// (att_stream_softmax_kernel.cu:28-71,136-191; note the scale is applied AFTER the max is subtracted, as there).
// `last` is clamped to ld: the reference's small kernels do the same by returning for threadIdx.x >= ld, its large
// kernel would run into the next row.  Every position of the row is written (the large reference kernel leaves
// [last, ld) untouched); a row with no valid position gives zeros.
__global__ __launch_bounds__(256) void att_stream_softmax_kernel(const float* __restrict__ x, const int32_t* __restrict__ dfn,
                                                                 const int32_t* __restrict__ mask_idx, int N, int ld,
                                                                 int cache_len, float scale, float* __restrict__ y,
                                                                 size_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int b = (int)(row / N);
  const int first = max(0, ld - dfn[b]);
  const int last = min(ld, min(ld, mask_idx[b]) + cache_len);
  const float* xr = x + row * ld;
  float* yr = y + row * ld;
  float mx = -FLT_MAX;
  for (int j = first + lane; j < last; j += 64) mx = fmaxf(mx, xr[j]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = first + lane; j < last; j += 64) sum += expf((xr[j] - mx) * scale);
  sum = wave_sum(sum);
  const float rz = 1.f / sum;
  for (int j = lane; j < ld; j += 64) yr[j] = (j >= first && j < last) ? expf((xr[j] - mx) * scale) * rz : 0.f;
}
int launch_att_stream_softmax(const float* scores, const int32_t* decode_frame_num, const int32_t* mask_idx, int B, int N,
                              int ld, int cache_len, float scale, float* out, hipStream_t stream) {
  M3_REQUIRE(B >= 0 && N >= 0 && ld > 0 && cache_len >= 0, "att_stream_softmax: bad shape");
  const size_t rows = (size_t)B * N;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(att_stream_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, scores,
                     decode_frame_num, mask_idx, N, ld, cache_len, scale, out, rows);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- RelPositionalEncoding (+ streaming offset)
// y = x * scale on (B,T,D); pos_emb = pe[off : off+T] with off = frame_num[0] (0 when frame_num is null: the full
// utterance form, rel_positional_encoding_kernel.cu:62-69); frame_num_out[b] = frame_num[b] + T.  The streaming kernel of
// the reference (:108-123) states this contract in its comment but still copies pe[0:T] and never advances the counter;
// the stated contract is what is implemented.
__global__ void rel_pos_enc_kernel(const float* __restrict__ x, const float* __restrict__ pe, const int32_t* __restrict__ frame_num,
                                   float scale, int B, int T, int D, float* __restrict__ y, float* __restrict__ pos_emb,
                                   int32_t* __restrict__ frame_num_out) {
  const size_t pos_n = (size_t)T * D, n = pos_n * B;
  const size_t off = frame_num ? (size_t)frame_num[0] * D : 0;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n; i += (size_t)gridDim.x * blockDim.x) {
    y[i] = x[i] * scale;
    if (i < pos_n) pos_emb[i] = pe[off + i];
  }
  if (frame_num && frame_num_out && tid < (size_t)B) frame_num_out[tid] = frame_num[tid] + T;
}
int launch_rel_positional_encoding(const float* x, const float* pe, int pe_len, const int32_t* frame_num, int max_offset,
                                   float scale, int B, int T, int D, float* y, float* pos_emb, int32_t* frame_num_out,
                                   hipStream_t stream) {
  M3_REQUIRE(B > 0 && T > 0 && D > 0, "rel_positional_encoding: empty problem");
  M3_REQUIRE((frame_num ? max_offset : 0) + T <= pe_len,
             "rel_positional_encoding: offset %d + %d frames exceeds the %d-position table", frame_num ? max_offset : 0, T, pe_len);
  // every work-group reads frame_num[0] as the offset, so the advanced counters go to a distinct buffer
  M3_REQUIRE(frame_num == nullptr || frame_num_out != frame_num, "rel_positional_encoding: frame_num_out must not alias frame_num");
  const size_t n = (size_t)B * T * D;
  hipLaunchKernelGGL(rel_pos_enc_kernel, dim3(grid1d(n, 2048)), dim3(256), 0, stream, x, pe, frame_num, scale, B, T, D, y,
                     pos_emb, frame_num_out);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
