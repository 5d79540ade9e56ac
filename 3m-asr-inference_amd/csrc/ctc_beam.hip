// Batched, resumable CTC prefix beam search on the device (trainer_3m_fix/model/encoder.py:182-275), and the streaming
// form of the greedy search (:156-180); behind them the endpoint detector that runs next to the two searches.
//
// Prefix beam search.  The input is m3_ctc_topk's (top_logp, top_idx) [B][T_chunk][k]; the recursion is the host routine's
// (decode.hip, ctc_prefix_beam_search_host) term for term, in double: the same log_add2 / log_add3 calls on the same operands in
// the same order, so that prefixes, their order and their scores come out as the host's.  One work-group per utterance; all
// frames of a call run inside one launch; the whole search state lives in caller-owned device memory, so a search can be
// resumed at any frame boundary (chunk by chunk gives the bits of one call over the concatenated frames).
//
// Per frame, with n beam entries and k candidate symbols, the host's slots are touched in the order
//   touch = (j * n + h) * 2 + sub      (j: top-k rank, h: beam position, sub = 1 only for the extension of "s == last")
// and a slot keeps its first touch as its tie-break in the stable second prune.  Two facts make the grouping small:
//   * an extension p + s can only coincide with a beam entry q (whose parent is p and whose last symbol is s) -- two
//     extensions never coincide, because the beam entries are distinct prefixes and the k symbols are distinct;
//   * so the slot of beam entry q receives at most three touches: the blank at rank jb (pb), the repeat of its last symbol
//     at rank jl (pnb), and its parent's extension by that same symbol (pnb); every other extension is a slot of its own.
// Candidates: the n beam-entry slots (if touched) and the n * k extension slots that did not merge.  The prune keeps the
// `beam` best by (score desc, first touch asc): each candidate counts the candidates ahead of it (its rank).
//
// Prefix identity.  Prefixes are nodes of a per-utterance trie (parent, token, depth).  Nodes are CANONICAL: a device hash
// table (parent, token) -> node holds every node ever made for the utterance, so a prefix that dropped out of the beam and
// is re-created later gets its old node back.  That is what makes "q's parent is p" (node compare) the same as "q == p + s"
// (prefix compare); with a fresh node per extension a re-created p would not be the parent of q and the same prefix would
// appear twice.  Only survivors of the prune get nodes: at most `beam` per frame, so the pool holds 1 + max_frames * beam.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace m3 {

namespace {

constexpr int kBeamMax = 32, kTopkMax = 32;
constexpr int kCandMax = kBeamMax + kBeamMax * kTopkMax;
constexpr int kBeamThreads = 256;
constexpr unsigned long long kEmptyKey = ~0ull;
// header words of one utterance's state
enum { H_STATUS = 0, H_FRAMES = 1, H_NCUR = 2, H_NNODES = 3, H_WORDS = 16 };

struct BeamLayout {       // byte offsets inside one utterance's slice of the state
  size_t beam_node, beam_pb, beam_pnb, parent, token, depth, hkey, hval, stride;
  int pool, hcap;
};

BeamLayout beam_layout(int beam, int max_frames) {
  BeamLayout L;
  L.pool = 1 + max_frames * beam;
  L.hcap = 16;
  while (L.hcap < 2 * L.pool) L.hcap <<= 1;
  size_t off = H_WORDS * 4;
  L.beam_node = off; off = align_up(off + (size_t)beam * 4, 8);
  L.beam_pb = off;   off += (size_t)beam * 8;
  L.beam_pnb = off;  off += (size_t)beam * 8;
  L.parent = off;    off = align_up(off + (size_t)L.pool * 4, 8);
  L.token = off;     off = align_up(off + (size_t)L.pool * 4, 8);
  L.depth = off;     off = align_up(off + (size_t)L.pool * 4, 8);
  L.hkey = off;      off += (size_t)L.hcap * 8;
  L.hval = off;      off += (size_t)L.hcap * 4;
  L.stride = align_up(off, 256);
  return L;
}

// Context biasing appends, behind the B slices above (which stay as they are, byte for byte), per utterance the context
// state and the bonus of every trie node: ctx_state[pool] int32, ctx_bonus[pool] double.
struct CtxLayout {
  size_t base, bonus, stride;   // base: offset of utterance 0's block in the state; bonus: offset of ctx_bonus in a block
};
CtxLayout ctx_layout(const BeamLayout& L, int B) {
  CtxLayout C;
  C.base = (size_t)B * L.stride;
  C.bonus = align_up((size_t)L.pool * 4, 8);
  C.stride = align_up(C.bonus + (size_t)L.pool * 8, 256);
  return C;
}

// LM fusion appends, behind the context blocks (which stay as they are, byte for byte), per utterance the LM state and the LM
// sum of every trie node: lm_state[pool] int32, lm_sum[pool] double -- the shape of a context block, so one layout type serves.
CtxLayout lm_layout(const BeamLayout& L, int B) {
  CtxLayout M = ctx_layout(L, B);
  M.base += (size_t)B * M.stride;
  return M;
}

int check_beam_desc(const m3_ctc_beam_desc* d) {
  M3_REQUIRE(d != nullptr, "ctc_beam: null descriptor");
  M3_REQUIRE(d->B >= 0, "ctc_beam: B = %d < 0", d->B);
  M3_REQUIRE(d->beam >= 1 && d->beam <= kBeamMax, "ctc_beam: beam = %d outside [1, %d]", d->beam, kBeamMax);
  M3_REQUIRE(d->k >= 1 && d->k <= kTopkMax, "ctc_beam: k = %d outside [1, %d]", d->k, kTopkMax);
  M3_REQUIRE(d->max_frames >= 0 && (int64_t)d->max_frames * d->beam < (1 << 28), "ctc_beam: max_frames = %d out of range",
             d->max_frames);
  M3_REQUIRE(d->blank >= 0, "ctc_beam: blank = %d < 0", d->blank);
  return 0;
}

// utils/common.py:148-156 in the form of decode.hip's host routine (std::max order, no contraction: -ffp-contract=off)
__device__ __forceinline__ double dmax(double a, double b) { return a < b ? b : a; }
__device__ __forceinline__ double log_add3(double a, double b, double c) {
  if (a == -INFINITY && b == -INFINITY && c == -INFINITY) return -INFINITY;
  const double m = dmax(a, dmax(b, c));
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}
__device__ __forceinline__ double log_add2(double a, double b) {
  if (a == -INFINITY && b == -INFINITY) return -INFINITY;
  const double m = dmax(a, b);
  return m + log(exp(a - m) + exp(b - m));
}

__device__ __forceinline__ unsigned long long node_key(int parent, int token) {
  return ((unsigned long long)(uint32_t)parent << 32) | (uint32_t)token;
}
__device__ __forceinline__ int hash_slot(unsigned long long key, int hcap) {
  key ^= key >> 33;
  key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33;
  return (int)(key & (unsigned long long)(hcap - 1));
}

struct BeamPtrs {
  int32_t* hdr;
  int32_t* node;
  double* pb;
  double* pnb;
  int32_t* parent;
  int32_t* token;
  int32_t* depth;
  unsigned long long* hkey;
  int32_t* hval;
};
__device__ __forceinline__ BeamPtrs beam_ptrs(const BeamLayout& L, char* state, int b) {
  char* s = state + (size_t)b * L.stride;
  return BeamPtrs{(int32_t*)s, (int32_t*)(s + L.beam_node), (double*)(s + L.beam_pb), (double*)(s + L.beam_pnb),
                  (int32_t*)(s + L.parent), (int32_t*)(s + L.token), (int32_t*)(s + L.depth),
                  (unsigned long long*)(s + L.hkey), (int32_t*)(s + L.hval)};
}

// grid (x: hash-table blocks, y: utterance): empty hash table, root node, beam = {empty prefix: pb = 0, pnb = -inf}
// slots != null: y indexes a device list of utterances (entries outside [0, B) are skipped)
__global__ __launch_bounds__(256) void ctc_beam_reset_kernel(BeamLayout L, char* state, const int32_t* __restrict__ slots, int B) {
  const int utt = slots != nullptr ? slots[blockIdx.y] : (int)blockIdx.y;
  if (utt < 0 || utt >= B) return;
  const BeamPtrs p = beam_ptrs(L, state, utt);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < L.hcap; i += gridDim.x * 256) {
    p.hkey[i] = kEmptyKey;
    p.hval[i] = -1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int w = 0; w < H_WORDS; ++w) p.hdr[w] = 0;
    p.hdr[H_NCUR] = 1;
    p.hdr[H_NNODES] = 1;
    p.parent[0] = -1;
    p.token[0] = -1;
    p.depth[0] = 0;
    p.node[0] = 0;
    p.pb[0] = 0.0;
    p.pnb[0] = -INFINITY;
  }
}

// What the biased search (CTX) adds to the advance; the unbiased instantiation takes an empty one and none of the CTX code.
struct CtxArgs {
  CtxLayout C;
  const int32_t* image;
  long long words;
  const int32_t* graph_of;
};
struct NoCtx {};
// What the fused search (LM) adds to the biased one.  M: the layout of the LM blocks (`bonus` is the offset of lm_sum).
struct LmArgs : CtxArgs {
  CtxLayout M;
  const int32_t* lm;
  long long lm_words;
  const int32_t* lm_on;
  double alpha, beta;
};
// A beam entry's back-off chain, staged in LDS once per frame: per level the arcs [lo, hi) and the weight gathered above it.
constexpr int kLmLevels = kLmMaxOrder, kLmW = kLmMaxOrder + 1;
__device__ __forceinline__ int ctx_in_range(int v, int n) { return (unsigned)v < (unsigned)n ? v : 0; }

// CTX: every trie node carries (context state, bonus), pure functions of its prefix; candidates are ranked by
// log_add2(pb, pnb) + bonus.  An utterance whose graph_of is outside [0, G) runs with state 0 and bonus 0.0 throughout.
// LM (on top of CTX): every trie node also carries (LM state, LM sum) of its prefix, and an utterance with lm_on != 0 and a
// well-formed LM image ranks by (log_add2(pb, pnb) + bonus) + (alpha lm + beta depth).  Per frame each beam entry's back-off
// chain is staged in LDS (wave 1, while wave 0 reads the frame), so an extension's walk (lm_step, kernels.h, term for term)
// goes to memory only for its binary-search probes and the arc it finds.  With lm_on == 0 nothing is added to the key.
template <bool CTX, class Ctx, bool LM = false>
__global__ __launch_bounds__(kBeamThreads) void ctc_beam_advance_kernel(BeamLayout L, int beam, int k, int blank, int max_frames,
                                                                        char* state, const float* __restrict__ top_logp,
                                                                        const int32_t* __restrict__ top_idx, int T_chunk,
                                                                        const int32_t* __restrict__ n_frames, Ctx cx) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const BeamPtrs p = beam_ptrs(L, state, b);
  // CTX only: the beam's and the survivors' (state, bonus), the frame's symbol classes, the utterance's graph
  __shared__ int s_state[CTX ? kBeamMax : 1], n_state[CTX ? kBeamMax : 1], f_cls[CTX ? kTopkMax : 1];
  __shared__ double s_bonus[CTX ? kBeamMax : 1], n_bonus[CTX ? kBeamMax : 1];
  __shared__ CtxGraph sh_g;
  __shared__ int sh_biased;
  int32_t* cs = nullptr;
  double* cb = nullptr;
  if constexpr (CTX) {
    char* c = state + cx.C.base + (size_t)b * cx.C.stride;
    cs = (int32_t*)c;
    cb = (double*)(c + cx.C.bonus);
  }
  // LM only: the beam's and the survivors' (LM state, LM sum), the staged chains, what each extension's walk found
  __shared__ int s_lst[LM ? kBeamMax : 1], n_lst[LM ? kBeamMax : 1], lv_n[LM ? kBeamMax : 1];
  __shared__ double s_lsum[LM ? kBeamMax : 1], n_lsum[LM ? kBeamMax : 1];
  __shared__ int lv_lo[LM ? kBeamMax * kLmLevels : 1], lv_hi[LM ? kBeamMax * kLmLevels : 1];
  __shared__ double lv_w[LM ? kBeamMax * kLmW : 1];
  __shared__ int c_lst[LM ? kBeamMax * kTopkMax : 1];
  __shared__ double c_lsum[LM ? kBeamMax * kTopkMax : 1];
  int32_t* ls = nullptr;
  double* lsm = nullptr;
  LmView lm{};
  bool fused = false;
  [[maybe_unused]] double alpha = 0.0;            // the utterance's LM weight: a set member's scale is folded in here, once
  if constexpr (LM) {                             // uniform: the header (a set's: and the directory entry) goes through the scalar cache
    char* c = state + cx.M.base + (size_t)b * cx.M.stride;
    ls = (int32_t*)c;
    lsm = (double*)(c + cx.M.bonus);
    alpha = cx.alpha;
    fused = lm_select(cx.lm, cx.lm_words, cx.lm_on[b], &lm, &alpha);
  }
  // current beam (best first) and its nodes
  __shared__ int s_node[kBeamMax], s_par[kBeamMax], s_tok[kBeamMax], s_dep[kBeamMax];
  __shared__ double s_pb[kBeamMax], s_pnb[kBeamMax];
  // this frame's candidates
  __shared__ int f_s[kTopkMax];
  __shared__ double f_ps[kTopkMax];
  __shared__ unsigned char merged[kBeamMax * kTopkMax];
  __shared__ double c_score[kCandMax], c_pb[kCandMax], c_pnb[kCandMax];
  __shared__ int c_first[kCandMax];
  // survivors, in rank order
  __shared__ int n_src[kBeamMax], n_node[kBeamMax], n_par[kBeamMax], n_tok[kBeamMax], n_dep[kBeamMax];
  __shared__ double n_pb[kBeamMax], n_pnb[kBeamMax];
  __shared__ int sh_status, sh_nf, sh_ncur, sh_nnodes, sh_nvalid;

  if (tid == 0) {
    int status = p.hdr[H_STATUS];
    const int frames = p.hdr[H_FRAMES];
    const int nf = min(max(n_frames[b], 0), T_chunk);
    if (status == 0 && frames + nf > max_frames) {     // nothing of this call is consumed; the state stays in bounds
      status = 1;
      p.hdr[H_STATUS] = status;
    }
    sh_status = status;
    sh_nf = nf;
    sh_ncur = p.hdr[H_NCUR];
    sh_nnodes = p.hdr[H_NNODES];
    if constexpr (CTX) sh_biased = ctx_graph_view(cx.image, cx.words, cx.graph_of[b], &sh_g) ? 1 : 0;
  }
  __syncthreads();
  if (sh_status != 0 || sh_nf == 0) return;
  const int nf = sh_nf;
  if (tid < sh_ncur) {
    const int nd = p.node[tid];
    s_node[tid] = nd;
    s_par[tid] = p.parent[nd];
    s_tok[tid] = p.token[nd];
    s_dep[tid] = p.depth[nd];
    s_pb[tid] = p.pb[tid];
    s_pnb[tid] = p.pnb[tid];
    if constexpr (CTX) {
      s_state[tid] = sh_biased ? ctx_in_range(cs[nd], sh_g.n_states) : 0;
      s_bonus[tid] = cb[nd];
    }
    if constexpr (LM) {                           // the root is in the LM's start state, whichever LM that is
      s_lst[tid] = fused ? (nd == 0 ? lm.start : lm_in_range(ls[nd], lm.n_states)) : 0;
      s_lsum[tid] = lsm[nd];
    }
  }
  if constexpr (LM) __syncthreads();
  int t = 0;
  for (; t < nf; ++t) {
    const int n = sh_ncur;
    const size_t row = ((size_t)b * T_chunk + t) * k;
    if (tid < k) {
      f_s[tid] = top_idx[row + tid];
      f_ps[tid] = (double)top_logp[row + tid];
      if constexpr (CTX) {                        // the frame's symbols are classed once
        const int s = f_s[tid];
        f_cls[tid] = sh_biased && (unsigned)s < (unsigned)sh_g.V ? ctx_in_range(sh_g.cls[s], sh_g.A) : 0;
      }
    }
    if constexpr (LM) {
      if (fused && tid >= 64 && tid < 64 + n) {
        const int h = tid - 64;
        int st = s_lst[h], l = 0;
        double w = 0.0;
        for (; st != 0 && l < kLmLevels; ++l) {
          int lo, hi;
          lm_arcs(lm, st, &lo, &hi);
          lv_lo[h * kLmLevels + l] = lo;
          lv_hi[h * kLmLevels + l] = hi;
          lv_w[h * kLmW + l] = w;
          w += (double)lm.bo_weight[st];
          const int nb = lm.bo_state[st];
          st = nb >= 0 && nb < st ? nb : 0;
        }
        lv_n[h] = l;
        lv_w[h * kLmW + l] = w;
      }
    }
    for (int i = tid; i < n * k; i += kBeamThreads) merged[i] = 0;
    if (tid == 0) sh_nvalid = 0;
    __syncthreads();
    // the slot of beam entry q: blank touch (pb), repeat touch and the parent's extension (pnb), in touch order
    if (tid < n) {
      const int q = tid, tok = s_tok[q];
      int jb = -1, jl = -1, ph = -1;
      for (int j = 0; j < k; ++j) {
        if (f_s[j] == blank) jb = j;
        if (f_s[j] == tok) jl = j;              // tok = -1 (root) never matches
      }
      for (int h = 0; h < n; ++h)
        if (s_node[h] == s_par[q]) ph = h;      // the root's parent (-1) never matches
      double pb = -INFINITY, pnb = -INFINITY;
      int first = 0x7fffffff;
      if (jb >= 0) {
        const double ps = f_ps[jb];
        pb = log_add3(pb, s_pb[q] + ps, s_pnb[q] + ps);
        first = (jb * n + q) * 2;
      }
      if (jl >= 0) {
        const double ps = f_ps[jl];
        const int rep = (jl * n + q) * 2;
        first = min(first, rep);
        if (ph >= 0) {
          const int sub = tok == s_tok[ph] ? 1 : 0;
          const int ext = (jl * n + ph) * 2 + sub;
          merged[ph * k + jl] = 1;
          first = min(first, ext);
          if (ext < rep) {
            pnb = sub ? log_add2(pnb, s_pb[ph] + ps) : log_add3(pnb, s_pb[ph] + ps, s_pnb[ph] + ps);
            pnb = log_add2(pnb, s_pnb[q] + ps);
          } else {
            pnb = log_add2(pnb, s_pnb[q] + ps);
            pnb = sub ? log_add2(pnb, s_pb[ph] + ps) : log_add3(pnb, s_pb[ph] + ps, s_pnb[ph] + ps);
          }
        } else {
          pnb = log_add2(pnb, s_pnb[q] + ps);
        }
      }
      c_pb[q] = pb;
      c_pnb[q] = pnb;
      c_first[q] = first;
      if (first != 0x7fffffff) {
        if constexpr (LM) {                       // ... and its LM sum
          double key = log_add2(pb, pnb) + s_bonus[q];
          if (fused) key = key + (alpha * s_lsum[q] + cx.beta * (double)s_dep[q]);
          c_score[q] = key;
        } else if constexpr (CTX) c_score[q] = log_add2(pb, pnb) + s_bonus[q];     // a beam entry's node holds its bonus
        else c_score[q] = log_add2(pb, pnb);
      }
    }
    __syncthreads();
    // the extensions that are slots of their own
    const int N = n + n * k;
    for (int i = tid; i < n * k; i += kBeamThreads) {
      const int h = i / k, j = i - h * k, c = n + i;
      const int s = f_s[j];
      if (s == blank || merged[i]) {
        c_first[c] = 0x7fffffff;
        continue;
      }
      const double ps = f_ps[j];
      double pnb;
      int sub;
      if (s == s_tok[h]) {
        sub = 1;
        pnb = log_add2(-INFINITY, s_pb[h] + ps);
      } else {
        sub = 0;
        pnb = log_add3(-INFINITY, s_pb[h] + ps, s_pnb[h] + ps);
      }
      c_pb[c] = -INFINITY;
      c_pnb[c] = pnb;
      c_first[c] = (j * n + h) * 2 + sub;
      if constexpr (CTX) {
        double bonus = s_bonus[h];
        if (sh_biased) bonus += (double)sh_g.delta[s_state[h] * sh_g.A + f_cls[j]];
        if constexpr (LM) {
          double key = log_add2(-INFINITY, pnb) + bonus;
          if (fused) {                            // lm_step from the staged chain
            const int nl = lv_n[h];
            int nx = 0, a = -1, l = 0;
            for (; l < nl; ++l) {
              a = lm_find(lm, lv_lo[h * kLmLevels + l], lv_hi[h * kLmLevels + l], s);
              if (a >= 0) break;
            }
            double lp;
            if (a >= 0) {
              nx = lm_in_range(lm.arc_next[a], lm.n_states);
              lp = lv_w[h * kLmW + l] + (double)lm.arc_logp[a];
            } else {
              lp = lm_step_root(lm, lv_w[h * kLmW + nl], s, &nx);
            }
            const double lsum = s_lsum[h] + lp;
            c_lst[i] = nx;
            c_lsum[i] = lsum;
            key = key + (alpha * lsum + cx.beta * (double)(s_dep[h] + 1));
          }
          c_score[c] = key;
        } else {
          c_score[c] = log_add2(-INFINITY, pnb) + bonus;
        }
      } else {
        c_score[c] = log_add2(-INFINITY, pnb);
      }
    }
    __syncthreads();
    // second prune: rank = number of candidates ahead in (score desc, first touch asc); ranks < beam survive
    for (int i = tid; i < N; i += kBeamThreads) {
      const int fi = c_first[i];
      if (fi == 0x7fffffff) continue;
      atomicAdd(&sh_nvalid, 1);
      const double si = c_score[i];
      int r = 0;
      for (int c = 0; c < N && r < beam; ++c) {
        const int fc = c_first[c];
        if (fc == 0x7fffffff) continue;
        const double sc = c_score[c];
        r += (sc > si || (sc == si && fc < fi)) ? 1 : 0;
      }
      if (r < beam) {
        n_src[r] = i;
        n_pb[r] = c_pb[i];
        n_pnb[r] = c_pnb[i];
      }
    }
    __syncthreads();
    // nodes of the survivors: a beam entry keeps its node; an extension looks (parent, token) up, or gets a new node
    if (tid < 64) {
      const int n_next = min(sh_nvalid, beam);
      int node = -1, par = -1, tok = -1, dep = 0;
      int cst = 0, ch = 0, cj = 0;                // CTX: the survivor's state and bonus; its parent and rank if an extension
      double cbo = 0.0;
      int lst = 0;                                // LM: the survivor's LM state and sum
      double lsum = 0.0;
      unsigned long long key = 0;
      if (tid < n_next) {
        const int src = n_src[tid];
        if (src < n) {
          node = s_node[src];
          par = s_par[src];
          tok = s_tok[src];
          dep = s_dep[src];
          if constexpr (CTX) {
            cst = s_state[src];
            cbo = s_bonus[src];
          }
          if constexpr (LM) {
            lst = s_lst[src];
            lsum = s_lsum[src];
          }
        } else {
          const int h = (src - n) / k, j = (src - n) - h * k;
          ch = h;
          cj = j;
          par = s_node[h];
          tok = f_s[j];
          dep = s_dep[h] + 1;
          key = node_key(par, tok);
          int slot = hash_slot(key, L.hcap);
          for (int probe = 0; probe < L.hcap; ++probe) {
            const unsigned long long kk = p.hkey[slot];
            if (kk == key) {
              node = p.hval[slot];
              break;
            }
            if (kk == kEmptyKey) break;
            slot = (slot + 1) & (L.hcap - 1);
          }
          if constexpr (CTX) {
            if (node >= 0) {                      // a prefix that was here before: its node still holds both
              cst = sh_biased ? ctx_in_range(cs[node], sh_g.n_states) : 0;
              cbo = cb[node];
            } else {
              cbo = s_bonus[ch];
              if (sh_biased) {
                const int arc = s_state[ch] * sh_g.A + f_cls[cj];
                cst = ctx_in_range(sh_g.next[arc], sh_g.n_states);
                cbo += (double)sh_g.delta[arc];
              }
            }
          }
          if constexpr (LM) {
            if (node >= 0) {
              lst = fused ? lm_in_range(ls[node], lm.n_states) : 0;
              lsum = lsm[node];
            } else if (fused) {
              lst = c_lst[src - n];
              lsum = c_lsum[src - n];
            }
          }
        }
      }
      const bool fresh = tid < n_next && node < 0;
      const unsigned long long m = __ballot(fresh);
      const int base = sh_nnodes;
      if (base + __popcll(m) > L.pool) {            // cannot happen while frames <= max_frames; never write past the pool
        if (tid == 0) sh_status = 2;
      } else if (fresh) {
        node = base + __popcll(m & ((1ull << tid) - 1ull));
        p.parent[node] = par;
        p.token[node] = tok;
        p.depth[node] = dep;
        if constexpr (CTX) {
          cs[node] = cst;
          cb[node] = cbo;
        }
        if constexpr (LM) {
          ls[node] = lst;
          lsm[node] = lsum;
        }
        int slot = hash_slot(key, L.hcap);
        for (int probe = 0; probe < L.hcap; ++probe) {
          if (atomicCAS(&p.hkey[slot], kEmptyKey, key) == kEmptyKey) {
            p.hval[slot] = node;
            break;
          }
          slot = (slot + 1) & (L.hcap - 1);
        }
      }
      if (tid < n_next) {
        n_node[tid] = node;
        n_par[tid] = par;
        n_tok[tid] = tok;
        n_dep[tid] = dep;
        if constexpr (CTX) {
          n_state[tid] = cst;
          n_bonus[tid] = cbo;
        }
        if constexpr (LM) {
          n_lst[tid] = lst;
          n_lsum[tid] = lsum;
        }
      }
      if (tid == 0) {
        sh_nnodes = base + (sh_status == 0 ? __popcll(m) : 0);
        sh_ncur = n_next;
      }
    }
    __syncthreads();
    if (sh_status != 0) break;
    if (tid < sh_ncur) {
      s_node[tid] = n_node[tid];
      s_par[tid] = n_par[tid];
      s_tok[tid] = n_tok[tid];
      s_dep[tid] = n_dep[tid];
      s_pb[tid] = n_pb[tid];
      s_pnb[tid] = n_pnb[tid];
      if constexpr (CTX) {
        s_state[tid] = n_state[tid];
        s_bonus[tid] = n_bonus[tid];
      }
      if constexpr (LM) {
        s_lst[tid] = n_lst[tid];
        s_lsum[tid] = n_lsum[tid];
      }
    }
    __syncthreads();
  }
  if (tid < sh_ncur && sh_status == 0) {
    p.node[tid] = s_node[tid];
    p.pb[tid] = s_pb[tid];
    p.pnb[tid] = s_pnb[tid];
  }
  if (tid == 0) {
    p.hdr[H_STATUS] = sh_status;
    if (sh_status == 0) {
      p.hdr[H_FRAMES] += nf;
      p.hdr[H_NCUR] = sh_ncur;
      p.hdr[H_NNODES] = sh_nnodes;
    }
  }
}

// the root's (state 0, bonus 0.0) of the listed utterances (slots == null: utterances 0 .. n - 1)
__global__ __launch_bounds__(256) void ctc_beam_ctx_reset_kernel(CtxLayout C, char* state, const int32_t* __restrict__ slots, int B,
                                                                 int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int utt = slots != nullptr ? slots[i] : i;
  if (utt < 0 || utt >= B) return;
  char* c = state + C.base + (size_t)utt * C.stride;
  ((int32_t*)c)[0] = 0;
  ((double*)(c + C.bonus))[0] = 0.0;
}

// ctc_beam_nbest_kernel plus the bonus: hypothesis r's final = bonus - pot[state]; rows are written in the order of
// (CTC score + final) desc, stable on the beam order; hyp_score stays the CTC score.
// LM: a fused utterance's key is (CTC score + final) + (alpha (lm + fin[lm_state] use_eos) + beta depth), and hyp_lm gets
// lm + fin[lm_state] use_eos (0 for an utterance that runs without the LM).
struct LmNbest {
  CtxLayout M;
  const int32_t* lm;
  long long lm_words;
  const int32_t* lm_on;
  double alpha, beta;
  int use_eos;
  float* hyp_lm;
};
struct NoLm {};
template <bool LM, class Lm>
__global__ __launch_bounds__(64) void ctc_beam_ctx_nbest_kernel(BeamLayout L, CtxLayout C, int beam, int max_frames,
                                                                const char* state, const int32_t* __restrict__ image,
                                                                long long words, const int32_t* __restrict__ graph_of,
                                                                int32_t* __restrict__ hyp_tokens, int32_t* __restrict__ hyp_len,
                                                                float* __restrict__ hyp_score, float* __restrict__ hyp_bonus,
                                                                int32_t* __restrict__ n_hyps, Lm lx) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const BeamPtrs p = beam_ptrs(L, (char*)state, b);
  const char* c = state + C.base + (size_t)b * C.stride;
  const int32_t* cs = (const int32_t*)c;
  const double* cb = (const double*)(c + C.bonus);
  __shared__ double key[kBeamMax];
  __shared__ int len_of[kBeamMax];
  const int status = p.hdr[H_STATUS];
  const int n = status ? 0 : min(p.hdr[H_NCUR], beam);
  int32_t* toks = hyp_tokens + (size_t)b * beam * max_frames;
  CtxGraph g;
  const bool biased = ctx_graph_view(image, words, graph_of[b], &g);
  double score = -INFINITY, fin = 0.0, lmf = 0.0;
  int nd = 0;
  LmView lm{};
  bool fused = false;
  [[maybe_unused]] double alpha = 0.0;
  if constexpr (LM) {
    alpha = lx.alpha;
    fused = lm_select(lx.lm, lx.lm_words, lx.lm_on[b], &lm, &alpha);
  }
  if (lane < n) {
    nd = p.node[lane];
    score = log_add2(p.pb[lane], p.pnb[lane]);
    fin = cb[nd];
    if (biased) fin -= (double)g.pot[ctx_in_range(cs[nd], g.n_states)];
    key[lane] = score + fin;
    if constexpr (LM) {
      if (fused) {
        const char* c2 = state + lx.M.base + (size_t)b * lx.M.stride;
        const int st = nd == 0 ? lm.start : lm_in_range(((const int32_t*)c2)[nd], lm.n_states);
        lmf = ((const double*)(c2 + lx.M.bonus))[nd] + (lx.use_eos ? (double)lm.fin[st] : 0.0);
        key[lane] = key[lane] + (alpha * lmf + lx.beta * (double)p.depth[nd]);
      }
    }
  }
  __syncthreads();
  if (lane < beam) {
    int r = lane, L_r = 0;
    if (lane < n) {
      r = 0;
      for (int i = 0; i < n; ++i) r += (key[i] > key[lane] || (key[i] == key[lane] && i < lane)) ? 1 : 0;
      L_r = min(p.depth[nd], max_frames);
      for (int i = L_r - 1; i >= 0 && nd > 0; --i) {
        toks[(size_t)r * max_frames + i] = p.token[nd];
        nd = p.parent[nd];
      }
    }
    len_of[r] = L_r;
    hyp_len[(size_t)b * beam + r] = L_r;
    hyp_score[(size_t)b * beam + r] = (float)score;
    hyp_bonus[(size_t)b * beam + r] = (float)fin;
    if constexpr (LM) lx.hyp_lm[(size_t)b * beam + r] = (float)lmf;
  }
  __syncthreads();
  for (int r = 0; r < beam; ++r)
    for (int i = len_of[r] + lane; i < max_frames; i += 64) toks[(size_t)r * max_frames + i] = -1;
  if (lane == 0) n_hyps[b] = status ? -1 : n;
}

// one wave per utterance; lane r < n_cur walks hypothesis r's trie path
__global__ __launch_bounds__(64) void ctc_beam_nbest_kernel(BeamLayout L, int beam, int max_frames, const char* state,
                                                            int32_t* __restrict__ hyp_tokens, int32_t* __restrict__ hyp_len,
                                                            float* __restrict__ hyp_score, int32_t* __restrict__ n_hyps) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const BeamPtrs p = beam_ptrs(L, (char*)state, b);
  const int status = p.hdr[H_STATUS];
  const int n = status ? 0 : min(p.hdr[H_NCUR], beam);
  int32_t* toks = hyp_tokens + (size_t)b * beam * max_frames;
  int L_r = 0;
  if (lane < beam) {
    float score = -INFINITY;
    if (lane < n) {
      int nd = p.node[lane];
      L_r = min(p.depth[nd], max_frames);
      for (int i = L_r - 1; i >= 0 && nd > 0; --i) {
        toks[(size_t)lane * max_frames + i] = p.token[nd];
        nd = p.parent[nd];
      }
      score = (float)log_add2(p.pb[lane], p.pnb[lane]);
    }
    hyp_len[(size_t)b * beam + lane] = L_r;
    hyp_score[(size_t)b * beam + lane] = score;
  }
  for (int r = 0; r < beam; ++r) {
    const int Lr = __shfl(L_r, r, 64);
    for (int i = Lr + lane; i < max_frames; i += 64) toks[(size_t)r * max_frames + i] = -1;
  }
  if (lane == 0) n_hyps[b] = status ? -1 : n;
}

// ---------------------------------------------------------------- streaming greedy search
// state per stream: [status, frames, previous frame's argmax (-1 before the first frame), token count] + tokens[max_frames]
enum { G_STATUS = 0, G_FRAMES = 1, G_PREV = 2, G_COUNT = 3, G_WORDS = 4 };

size_t greedy_stride(int max_frames) { return align_up((size_t)(G_WORDS + max_frames) * 4, 256) / 4; }

int check_greedy_desc(const m3_ctc_greedy_desc* d) {
  M3_REQUIRE(d != nullptr, "ctc_greedy_stream: null descriptor");
  M3_REQUIRE(d->B >= 0 && d->max_frames >= 0 && d->blank >= 0, "ctc_greedy_stream: bad descriptor B=%d max_frames=%d blank=%d",
             d->B, d->max_frames, d->blank);
  return 0;
}

__global__ __launch_bounds__(256) void ctc_greedy_stream_reset_kernel(int32_t* state, size_t stride, int B,
                                                                      const int32_t* __restrict__ slots, int n) {
  int b = blockIdx.x * 256 + threadIdx.x;
  if (slots != nullptr) {                         // a device list of n streams (entries outside [0, B) are skipped)
    if (b >= n) return;
    b = slots[b];
    if (b < 0) return;
  }
  if (b >= B) return;
  int32_t* st = state + (size_t)b * stride;
  st[G_STATUS] = 0;
  st[G_FRAMES] = 0;
  st[G_PREV] = -1;
  st[G_COUNT] = 0;
}

// one wave per stream: ctc_collapse_kernel with the previous frame's id carried across calls
__global__ __launch_bounds__(64) void ctc_greedy_stream_kernel(const int32_t* __restrict__ ids, int T_chunk,
                                                               const int32_t* __restrict__ n_frames, int blank, int max_frames,
                                                               int32_t* state, size_t stride) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int32_t* st = state + (size_t)b * stride;
  int32_t* out = st + G_WORDS;
  const int nf = min(max(n_frames[b], 0), T_chunk);
  const int status = st[G_STATUS], frames = st[G_FRAMES], prev = st[G_PREV];
  int count = st[G_COUNT];
  if (status != 0 || frames + nf > max_frames) {
    if (lane == 0) st[G_STATUS] = status ? status : 1;
    return;
  }
  const int32_t* row = ids + (size_t)b * T_chunk;
  for (int t0 = 0; t0 < nf; t0 += 64) {
    const int t = t0 + lane;
    bool keep = false;
    int id = blank;
    if (t < nf) {
      id = row[t];
      keep = id != blank && id != (t == 0 ? prev : row[t - 1]);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) out[count + __popcll(m & ((1ull << lane) - 1ull))] = id;
    count += __popcll(m);
  }
  if (lane == 0) {
    st[G_FRAMES] = frames + nf;
    if (nf > 0) st[G_PREV] = row[nf - 1];
    st[G_COUNT] = count;
  }
}

__global__ __launch_bounds__(64) void ctc_greedy_stream_tokens_kernel(const int32_t* state, size_t stride, int max_frames,
                                                                      int32_t* __restrict__ tokens, int32_t* __restrict__ n_tokens) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t* st = state + (size_t)b * stride;
  const int status = st[G_STATUS];
  const int count = status ? 0 : st[G_COUNT];
  for (int i = lane; i < max_frames; i += 64) tokens[(size_t)b * max_frames + i] = i < count ? st[G_WORDS + i] : -1;
  if (lane == 0) n_tokens[b] = status ? -1 : count;
}


// ---------------------------------------------------------------- endpoint detection
// state per stream (and a row of m3_ctc_endpoint_read's info): the seven values of the rule and one spare word
enum { E_FRAMES = 0, E_TRAIL = 1, E_DECODED = 2, E_FIRST = 3, E_LAST = 4, E_RULE = 5, E_FIRED = 6, E_SPARE = 7, E_WORDS = 8 };

int check_endpoint_desc(const m3_ctc_endpoint_desc* d) {
  M3_REQUIRE(d != nullptr, "ctc_endpoint: null descriptor");
  M3_REQUIRE(d->B >= 0 && d->B <= (1 << 24), "ctc_endpoint: B = %d outside [0, 2^24]", d->B);
  M3_REQUIRE(d->blank >= 0, "ctc_endpoint: blank = %d < 0", d->blank);
  M3_REQUIRE(d->n_rules >= 1 && d->n_rules <= 4, "ctc_endpoint: n_rules = %d outside [1, 4]", d->n_rules);
  // a blank above p = 0.5 is the frame's argmax, so entry 0 of any top-k decides; NaN fails both comparisons
  M3_REQUIRE(d->log_blank_threshold >= (float)std::log(0.5) && d->log_blank_threshold < 0.0f,
             "ctc_endpoint: log_blank_threshold = %g outside [log 0.5, 0)", (double)d->log_blank_threshold);
  for (int r = 0; r < d->n_rules; ++r)
    M3_REQUIRE((d->rule[r].must_decoded == 0 || d->rule[r].must_decoded == 1) && d->rule[r].min_trailing >= 0 &&
                   d->rule[r].min_length >= 0,
               "ctc_endpoint: rule %d = (%d, %d, %d): must_decoded is 0 or 1, the frame counts are >= 0", r + 1,
               d->rule[r].must_decoded, d->rule[r].min_trailing, d->rule[r].min_length);
  return 0;
}

__global__ __launch_bounds__(256) void ctc_endpoint_reset_kernel(int32_t* state, int B, const int32_t* __restrict__ slots, int n) {
  int b = blockIdx.x * 256 + threadIdx.x;
  if (slots != nullptr) {                         // a device list of n streams (entries outside [0, B) are skipped)
    if (b >= n) return;
    b = slots[b];
    if (b < 0) return;
  }
  if (b >= B) return;
  int32_t* st = state + (size_t)b * E_WORDS;
  st[E_FRAMES] = 0;
  st[E_TRAIL] = 0;
  st[E_DECODED] = 0;
  st[E_FIRST] = -1;
  st[E_LAST] = -1;
  st[E_RULE] = 0;
  st[E_FIRED] = -1;
  st[E_SPARE] = 0;
}

// What a stream's state is after lane L of an iteration, from the state before the iteration's lane 0 and the two ballots.
// Lanes 0 .. L hold real frames (the caller asks only for those), so a clear bit of `blank` at or below L is a frame that
// ends the run of blanks.
struct EpState {
  int frames, trail, decoded, first, last;
};
__device__ __forceinline__ EpState ep_after_lane(const EpState& c, unsigned long long blank, unsigned long long speech, int L) {
  const unsigned long long upto = L >= 63 ? ~0ull : (1ull << (L + 1)) - 1ull;      // lanes 0 .. L
  const unsigned long long stop = ~blank & upto, sp = speech & upto;
  EpState s;
  s.frames = c.frames + L + 1;
  s.trail = stop ? L - (63 - __clzll((long long)stop)) : c.trail + L + 1;
  s.decoded = (c.decoded || sp) ? 1 : 0;
  s.first = c.first >= 0 || !sp ? c.first : c.frames + (__ffsll((long long)sp) - 1);
  s.last = sp ? c.frames + (63 - __clzll((long long)sp)) : c.last;
  return s;
}

// one wave per stream, 64 frames per iteration: every lane works out the state after its own frame and evaluates the rules
// there; the first lane on which a rule fires ends the call for this stream
__global__ __launch_bounds__(64) void ctc_endpoint_advance_kernel(m3_ctc_endpoint_desc d, int32_t* state,
                                                                  const float* __restrict__ top_logp,
                                                                  const int32_t* __restrict__ top_idx, int T_chunk, int k,
                                                                  const int32_t* __restrict__ n_frames) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int32_t* st = state + (size_t)b * E_WORDS;
  const int nf = min(max(n_frames[b], 0), T_chunk);
  if (nf == 0 || st[E_RULE] != 0) return;         // idle, or latched: the state stays word for word
  EpState c{st[E_FRAMES], st[E_TRAIL], st[E_DECODED], st[E_FIRST], st[E_LAST]};
  int rule = 0;
  for (int t0 = 0; t0 < nf; t0 += 64) {
    const int t = t0 + lane, n_it = min(nf - t0, 64);
    bool is_blank = false, is_speech = false;
    if (t < nf) {                                 // rows past nf are padding and are not read
      const size_t e0 = ((size_t)b * T_chunk + t) * k;
      const int id = top_idx[e0];
      is_speech = id != d.blank;
      is_blank = !is_speech && top_logp[e0] > d.log_blank_threshold;
    }
    const unsigned long long mb = __ballot(is_blank), ms = __ballot(is_speech);
    int fired = 0;
    if (t < nf) {
      const EpState s = ep_after_lane(c, mb, ms, lane);
#pragma unroll
      for (int r = 3; r >= 0; --r)
        if (r < d.n_rules && (s.decoded || !d.rule[r].must_decoded) && s.trail >= d.rule[r].min_trailing &&
            s.frames >= d.rule[r].min_length)
          fired = r + 1;                          // descending r: the lowest rule that fires stays
    }
    const unsigned long long mf = __ballot(fired != 0);
    if (mf) {                                     // frames behind the first firing lane are ignored
      const int L = __ffsll((long long)mf) - 1;
      rule = __shfl(fired, L, 64);
      c = ep_after_lane(c, mb, ms, L);
      break;
    }
    c = ep_after_lane(c, mb, ms, n_it - 1);
  }
  if (lane == 0) {
    st[E_FRAMES] = c.frames;
    st[E_TRAIL] = c.trail;
    st[E_DECODED] = c.decoded;
    st[E_FIRST] = c.first;
    st[E_LAST] = c.last;
    if (rule) {
      st[E_RULE] = rule;
      st[E_FIRED] = c.frames - 1;
    }
  }
}

__global__ __launch_bounds__(256) void ctc_endpoint_read_kernel(const int32_t* __restrict__ state, int32_t* __restrict__ info, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) info[i] = state[i];
}

// ---------------------------------------------------------------- the host half of the prefix beam search
// An entry point (api.hip) says which form it is and fills a BeamCall; check_call holds every rule of the twelve launching entry
// points in the order each of them had, and beam_reset / beam_advance / beam_nbest hold the launches.

// bytes of state: the B slices; behind them (Ctx) a context block per utterance; behind those (Lm) an LM block per utterance
size_t state_need(const m3_ctc_beam_desc& d, BeamForm form) {
  const BeamLayout L = beam_layout(d.beam, d.max_frames);
  if (form == BeamForm::Plain) return (size_t)d.B * L.stride;
  const CtxLayout last = form == BeamForm::Ctx ? ctx_layout(L, d.B) : lm_layout(L, d.B);
  return last.base + (size_t)d.B * last.stride;
}

int check_ctx_image(const char* who, const void* image, size_t image_bytes, const int32_t* graph_of) {
  M3_REQUIRE(graph_of != nullptr, "%s: null graph_of", who);
  M3_REQUIRE(image != nullptr || image_bytes == 0, "%s: null image of %zu bytes", who, image_bytes);
  M3_REQUIRE(image_bytes % 4 == 0 && image_bytes <= kCtxMaxBytes && (image == nullptr || image_bytes >= CTX_HDR_WORDS * 4),
             "%s: image of %zu bytes (a multiple of 4 in [%d, %zu])", who, image_bytes, CTX_HDR_WORDS * 4, kCtxMaxBytes);
  return 0;
}

int check_lm_image(const char* who, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha, double beta) {
  M3_REQUIRE(lm_on != nullptr, "%s: null lm_on", who);
  M3_REQUIRE(lm_image != nullptr || lm_bytes == 0, "%s: null LM image of %zu bytes", who, lm_bytes);
  // a single image or a set: which one only the device copy says, so the bound is the set's
  M3_REQUIRE(lm_bytes % 4 == 0 && lm_bytes <= kLmSetMaxBytes && (lm_image == nullptr || lm_bytes >= LM_HDR_WORDS * 4),
             "%s: LM image of %zu bytes (a multiple of 4 in [%d, %zu])", who, lm_bytes, LM_HDR_WORDS * 4, kLmSetMaxBytes);
  M3_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "%s: alpha or beta is not finite", who);
  return 0;
}

enum class BeamOp { Reset, Advance, Nbest };
constexpr int kLaunch = 1;
// < 0: refused; 0: nothing to do (no utterance, no frame, an empty slot list); kLaunch: go on.
// The order and the words are the exports' (tests/test_ctc_beam_refusals_host.py pins them).  Two of them are not what one would
// write today: the plain reset looks at the slot list before the state, the biased and the fused reset at their state first; and
// all three refuse a bad slot list in the plain reset's name.
int check_call(const BeamCall& c, BeamOp op) {
  if (int rc = check_beam_desc(c.d)) return rc;
  const m3_ctc_beam_desc& d = *c.d;
  const bool ctx = c.form != BeamForm::Plain, lm = c.form == BeamForm::Lm;
  const bool slots_ok = c.n >= 0 && (c.slots != nullptr || c.n == 0);
  if (op == BeamOp::Reset && !ctx) M3_REQUIRE(slots_ok, "ctc_beam_reset: bad slot list");
  const size_t need = state_need(d, c.form);
  M3_REQUIRE(c.state != nullptr && c.bytes >= need, "%s: state %zu bytes < required %zu", c.who, c.bytes, need);
  if (op == BeamOp::Reset) M3_REQUIRE(slots_ok, "ctc_beam_reset: bad slot list");
  if (op == BeamOp::Advance) M3_REQUIRE(c.T_chunk >= 0, "%s: T_chunk = %d < 0", c.who, c.T_chunk);
  if (d.B == 0 || (op == BeamOp::Advance && c.T_chunk == 0) || (op == BeamOp::Reset && c.slots != nullptr && c.n == 0)) return 0;
  if (op == BeamOp::Reset) return kLaunch;
  if (op == BeamOp::Advance) M3_REQUIRE(c.top_logp && c.top_idx && c.n_frames, "%s: null pointer", c.who);
  if (op == BeamOp::Nbest)
    M3_REQUIRE(c.hyp_len && c.hyp_score && (c.hyp_bonus || !ctx) && (c.hyp_lm || !lm) && c.n_hyps && (c.hyp_tokens || d.max_frames == 0),
               "%s: null pointer", c.who);
  if (ctx)
    if (int rc = check_ctx_image(c.who, c.image, c.image_bytes, c.graph_of)) return rc;
  if (lm)
    if (int rc = check_lm_image(c.who, c.lm_image, c.lm_bytes, c.lm_on, c.alpha, c.beta)) return rc;
  return kLaunch;
}

}  // namespace

size_t beam_state_need(const m3_ctc_beam_desc* d, BeamForm form) { return check_beam_desc(d) ? 0 : state_need(*d, form); }

int beam_reset(const BeamCall& c) {
  const int rc = check_call(c, BeamOp::Reset);
  if (rc != kLaunch) return rc;
  const m3_ctc_beam_desc& d = *c.d;
  const BeamLayout L = beam_layout(d.beam, d.max_frames);
  const int cnt = c.slots ? c.n : d.B;
  const unsigned gx = (unsigned)std::min((L.hcap + 255) / 256, 64);
  hipLaunchKernelGGL(ctc_beam_reset_kernel, dim3(gx, cnt), dim3(256), 0, c.stream, L, (char*)c.state, c.slots, d.B);
  M3_LAUNCH_CHECK();
  // the root's (context state, bonus), then its (LM state, LM sum): the context block's kernel, on the LM blocks too
  const CtxLayout blocks[2] = {ctx_layout(L, d.B), lm_layout(L, d.B)};
  const int n_blocks = c.form == BeamForm::Plain ? 0 : c.form == BeamForm::Ctx ? 1 : 2;
  for (int i = 0; i < n_blocks; ++i) {
    hipLaunchKernelGGL(ctc_beam_ctx_reset_kernel, dim3((cnt + 255) / 256), dim3(256), 0, c.stream, blocks[i], (char*)c.state, c.slots,
                       d.B, cnt);
    M3_LAUNCH_CHECK();
  }
  return 0;
}

int beam_advance(const BeamCall& c) {
  const int rc = check_call(c, BeamOp::Advance);
  if (rc != kLaunch) return rc;
  const m3_ctc_beam_desc& d = *c.d;
  const BeamLayout L = beam_layout(d.beam, d.max_frames);
  LmArgs cx;                                      // the biased form takes the CtxArgs in it
  cx.C = ctx_layout(L, d.B);
  cx.image = (const int32_t*)c.image;
  cx.words = (long long)(c.image_bytes / 4);
  cx.graph_of = c.graph_of;
  cx.M = lm_layout(L, d.B);
  cx.lm = (const int32_t*)c.lm_image;
  cx.lm_words = (long long)(c.lm_bytes / 4);
  cx.lm_on = c.lm_on;
  cx.alpha = c.alpha;
  cx.beta = c.beta;
  const dim3 grid(d.B), block(kBeamThreads);
  char* state = (char*)c.state;
  switch (c.form) {
    case BeamForm::Plain:
      hipLaunchKernelGGL((ctc_beam_advance_kernel<false, NoCtx>), grid, block, 0, c.stream, L, d.beam, d.k, d.blank, d.max_frames, state,
                         c.top_logp, c.top_idx, c.T_chunk, c.n_frames, NoCtx{});
      break;
    case BeamForm::Ctx:
      hipLaunchKernelGGL((ctc_beam_advance_kernel<true, CtxArgs>), grid, block, 0, c.stream, L, d.beam, d.k, d.blank, d.max_frames, state,
                         c.top_logp, c.top_idx, c.T_chunk, c.n_frames, (const CtxArgs&)cx);
      break;
    case BeamForm::Lm:
      hipLaunchKernelGGL((ctc_beam_advance_kernel<true, LmArgs, true>), grid, block, 0, c.stream, L, d.beam, d.k, d.blank, d.max_frames,
                         state, c.top_logp, c.top_idx, c.T_chunk, c.n_frames, cx);
      break;
  }
  M3_LAUNCH_CHECK();
  return 0;
}

int beam_nbest(const BeamCall& c) {
  const int rc = check_call(c, BeamOp::Nbest);
  if (rc != kLaunch) return rc;
  const m3_ctc_beam_desc& d = *c.d;
  const BeamLayout L = beam_layout(d.beam, d.max_frames);
  const CtxLayout C = ctx_layout(L, d.B);
  const int32_t* image = (const int32_t*)c.image;
  const long long words = (long long)(c.image_bytes / 4);
  const char* state = (const char*)c.state;
  const LmNbest lx{lm_layout(L, d.B), (const int32_t*)c.lm_image, (long long)(c.lm_bytes / 4), c.lm_on, c.alpha, c.beta,
                   c.use_eos ? 1 : 0, c.hyp_lm};
  switch (c.form) {
    case BeamForm::Plain:
      hipLaunchKernelGGL(ctc_beam_nbest_kernel, dim3(d.B), dim3(64), 0, c.stream, L, d.beam, d.max_frames, state, c.hyp_tokens, c.hyp_len,
                         c.hyp_score, c.n_hyps);
      break;
    case BeamForm::Ctx:
      hipLaunchKernelGGL((ctc_beam_ctx_nbest_kernel<false, NoLm>), dim3(d.B), dim3(64), 0, c.stream, L, C, d.beam, d.max_frames, state,
                         image, words, c.graph_of, c.hyp_tokens, c.hyp_len, c.hyp_score, c.hyp_bonus, c.n_hyps, NoLm{});
      break;
    case BeamForm::Lm:
      hipLaunchKernelGGL((ctc_beam_ctx_nbest_kernel<true, LmNbest>), dim3(d.B), dim3(64), 0, c.stream, L, C, d.beam, d.max_frames, state,
                         image, words, c.graph_of, c.hyp_tokens, c.hyp_len, c.hyp_score, c.hyp_bonus, c.n_hyps, lx);
      break;
  }
  M3_LAUNCH_CHECK();
  return 0;
}

size_t ctc_greedy_stream_state_size(const m3_ctc_greedy_desc* d) {
  if (check_greedy_desc(d)) return 0;
  return (size_t)d->B * greedy_stride(d->max_frames) * 4;
}

int launch_ctc_greedy_stream_reset(const m3_ctc_greedy_desc* d, void* state, size_t bytes, hipStream_t stream, const int32_t* slots,
                                   int n) {
  if (int rc = check_greedy_desc(d)) return rc;
  M3_REQUIRE(n >= 0 && (slots != nullptr || n == 0), "ctc_greedy_stream_reset: bad slot list");
  if (slots != nullptr && n == 0) return 0;
  const size_t stride = greedy_stride(d->max_frames);
  M3_REQUIRE(state != nullptr && bytes >= (size_t)d->B * stride * 4, "ctc_greedy_stream_reset: state %zu bytes < required %zu",
             bytes, (size_t)d->B * stride * 4);
  if (d->B == 0) return 0;
  hipLaunchKernelGGL(ctc_greedy_stream_reset_kernel, dim3(((slots ? n : d->B) + 255) / 256), dim3(256), 0, stream, (int32_t*)state,
                     stride, d->B, slots, n);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_ctc_greedy_stream_advance(const m3_ctc_greedy_desc* d, void* state, size_t bytes, const float* logits, int T_chunk,
                                     int V, const int32_t* n_frames, int32_t* frame_ids, hipStream_t stream) {
  if (int rc = check_greedy_desc(d)) return rc;
  const size_t stride = greedy_stride(d->max_frames);
  M3_REQUIRE(state != nullptr && bytes >= (size_t)d->B * stride * 4, "ctc_greedy_stream_advance: state %zu bytes < required %zu",
             bytes, (size_t)d->B * stride * 4);
  M3_REQUIRE(T_chunk >= 0 && V > 0, "ctc_greedy_stream_advance: bad shape T_chunk=%d V=%d", T_chunk, V);
  if (d->B == 0 || T_chunk == 0) return 0;
  M3_REQUIRE(logits && n_frames && frame_ids, "ctc_greedy_stream_advance: null pointer");
  if (int rc = launch_ctc_argmax(logits, (size_t)d->B * T_chunk, V, frame_ids, stream)) return rc;
  hipLaunchKernelGGL(ctc_greedy_stream_kernel, dim3(d->B), dim3(64), 0, stream, frame_ids, T_chunk, n_frames, d->blank,
                     d->max_frames, (int32_t*)state, stride);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_ctc_greedy_stream_tokens(const m3_ctc_greedy_desc* d, const void* state, size_t bytes, int32_t* tokens,
                                    int32_t* n_tokens, hipStream_t stream) {
  if (int rc = check_greedy_desc(d)) return rc;
  const size_t stride = greedy_stride(d->max_frames);
  M3_REQUIRE(state != nullptr && bytes >= (size_t)d->B * stride * 4, "ctc_greedy_stream_tokens: state %zu bytes < required %zu",
             bytes, (size_t)d->B * stride * 4);
  if (d->B == 0) return 0;
  M3_REQUIRE(n_tokens && (tokens || d->max_frames == 0), "ctc_greedy_stream_tokens: null pointer");
  hipLaunchKernelGGL(ctc_greedy_stream_tokens_kernel, dim3(d->B), dim3(64), 0, stream, (const int32_t*)state, stride,
                     d->max_frames, tokens, n_tokens);
  M3_LAUNCH_CHECK();
  return 0;
}

size_t ctc_endpoint_state_size(const m3_ctc_endpoint_desc* d) {
  if (check_endpoint_desc(d)) return 0;
  return (size_t)d->B * E_WORDS * 4;
}

int launch_ctc_endpoint_reset(const m3_ctc_endpoint_desc* d, void* state, size_t bytes, hipStream_t stream, const int32_t* slots,
                              int n) {
  if (int rc = check_endpoint_desc(d)) return rc;
  M3_REQUIRE(n >= 0 && (slots != nullptr || n == 0), "ctc_endpoint_reset: bad slot list");
  if (slots != nullptr && n == 0) return 0;
  M3_REQUIRE(bytes >= (size_t)d->B * E_WORDS * 4, "ctc_endpoint_reset: state %zu bytes < required %zu", bytes,
             (size_t)d->B * E_WORDS * 4);
  if (d->B == 0) return 0;
  M3_REQUIRE(state != nullptr, "ctc_endpoint_reset: null state");
  hipLaunchKernelGGL(ctc_endpoint_reset_kernel, dim3(((slots ? n : d->B) + 255) / 256), dim3(256), 0, stream, (int32_t*)state,
                     d->B, slots, n);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_ctc_endpoint_advance(const m3_ctc_endpoint_desc* d, void* state, size_t bytes, const float* top_logp,
                                const int32_t* top_idx, int T_chunk, int k, const int32_t* n_frames, hipStream_t stream) {
  if (int rc = check_endpoint_desc(d)) return rc;
  M3_REQUIRE(bytes >= (size_t)d->B * E_WORDS * 4, "ctc_endpoint_advance: state %zu bytes < required %zu", bytes,
             (size_t)d->B * E_WORDS * 4);
  M3_REQUIRE(T_chunk >= 0 && k >= 1, "ctc_endpoint_advance: bad shape T_chunk=%d k=%d", T_chunk, k);
  if (d->B == 0 || T_chunk == 0) return 0;
  M3_REQUIRE(state && top_logp && top_idx && n_frames, "ctc_endpoint_advance: null pointer");
  hipLaunchKernelGGL(ctc_endpoint_advance_kernel, dim3(d->B), dim3(64), 0, stream, *d, (int32_t*)state, top_logp, top_idx, T_chunk,
                     k, n_frames);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_ctc_endpoint_read(const m3_ctc_endpoint_desc* d, const void* state, size_t bytes, int32_t* info, hipStream_t stream) {
  if (int rc = check_endpoint_desc(d)) return rc;
  M3_REQUIRE(bytes >= (size_t)d->B * E_WORDS * 4, "ctc_endpoint_read: state %zu bytes < required %zu", bytes,
             (size_t)d->B * E_WORDS * 4);
  if (d->B == 0) return 0;
  M3_REQUIRE(state && info, "ctc_endpoint_read: null pointer");
  const int n = d->B * E_WORDS;
  hipLaunchKernelGGL(ctc_endpoint_read_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const int32_t*)state, info, n);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
