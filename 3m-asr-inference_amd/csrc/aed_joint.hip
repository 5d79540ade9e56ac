// The fused step of the attention beam search: a score and a prune launch that take the place of
// m3_aed_search_prune behind the output layer and rank every candidate by its attention log-probability plus up to three parts:
// its CTC prefix probability (CTC), an n-gram LM's (LM), a context graph's bonus (CTX).  ONE score and ONE prune kernel template on
// <CTC, LM, CTX, Lx> serve the seven forms with at least one part; three families of entry points (m3_aed_joint_*, m3_aed_ngram_*,
// m3_aed_bias_*) reach them through one call record, one check and one launch table (the host half at the end of this file).
//
// CTC (m3_aed_joint_*): every candidate is also scored by its CTC PREFIX probability (Watanabe et al. 2017) and
// ranked by  key = (1 - w) att + w ctc.  The kernels work on the SAME search state (aed_search_state.h: headers, double-buffered
// records, token and ancestry paths; the record's score word holds the joint key) plus two blobs of their own:
//
//   scorer state (fp32 words), per row r, double-buffered by the parity of its utterance's step like the records:
//       [ att, ctc (= psi of the hypothesis), 0, 0, rn[F], rb[F] ]      F = max_frames
//     rn[t] / rb[t]: log-probability of the alignments of frames 0 .. t that collapse to the hypothesis and end in its last
//     token / in blank.  Only t < m (the utterance's frames) is ever read.
//   scratch, rewritten by every step:
//       candidate records [R][K][4]: token, att', ctc', key       K = pre_beam; key = NaN: no such candidate
//       candidate states  [R][F][2][K]: rn' | rb' of candidate j of row r at frame t (lane j writes K contiguous floats)
//
// m3_aed_joint_prune COPIES the survivors' states from the scratch; it does not recompute them.  The copy is N * 2 m words per
// utterance spread over 256 threads, against a second serial chain of m dependent log-add-exps on B work-groups, and a copy
// cannot differ from what was scored.
//
// fp32, no atomics, every reduction in a fixed order, a row's result independent of its place in the batch.  No work-group
// reads a word that another one writes in the same launch: score reads buffer `step & 1` and writes only its row's scratch;
// prune reads the scratch and writes the other buffer.  A done utterance is left bit for bit alone in all blobs.
//
// LM: N-GRAM LM FUSION AND THE LENGTH BONUS (m3_aed_ngram_*).  Every candidate also takes one step through the LM
// image of kernels.h (lm_step's terms in lm_step's order) and  key = jkey + (float)(alpha lm' + beta n'),  jkey the joint key above;
// with CTC = false (ctc_weight = 0) there is no scorer state, no frame chain, the ctc part is 0 and jkey = att'.  Two more blobs:
//
//   LM state (int32 words), per row, double-buffered like the records:  [ lm_state, n, lm (double, 2 words), att, 0, 0, 0 ]
//     att is the attention part, kept here only by the CTC = false form (it has no scorer state to keep it in).
//   LM scratch: [R][K] of [ lm_state', 0, lm' (double) ], then [R][K][4] candidate records of the CTC = false form (the CTC
//     form's records stay in the joint scratch).
//
// Prune copies the survivors' (lm_state', lm') from the scratch: nothing is walked twice.  An utterance whose lm_on is 0 (or
// whose image fails lm_view) adds nothing: its keys, parts, records and scorer states are the joint step's bits.
//
// CTX: HOTWORD BIASING (m3_aed_bias_*).  Every candidate also takes one arc of its utterance's context graph
// (kernels.h ctx_graph_view; the image, its compiler and its validator are the CTC search's) and
//   key = jkey + (float)extra,   extra = (alpha lm' + beta n') + bonus' with an LM, bonus' without,   in double, rounded once.
// A token adds delta[state][cls[token]] and moves to next[state][..]; eos hands back pot[state] and ends in state 0.
// Two more blobs, sized by B, beam and pre_beam alone:
//
//   context state (int32 words), per row, double-buffered like the records:  [ ctx_state, att, bonus (double, 2 words) ]
//     att is kept here only by the <false, false, true> form, which has neither a scorer state nor an LM state to keep it in.
//   context scratch: [R][K] of [ ctx_state', 0, bonus' (double) ], then [R][K][4] candidate records of the <false, false, true> form.
//
// Prune copies the survivors' (ctx_state', bonus') from the scratch.  An utterance whose graph_of is outside [0, G) (or whose
// image fails ctx_graph_view or was built for another V) adds nothing and carries (0, 0.0) along.
//
// WHERE THE FORM IS DECIDED.  An entry point says which parts its call has (FusedCall::ctc / lm / ctx, from its family,
// ctc_weight and which optional pointers are given); check_call checks exactly those parts' blobs, and launch_fused picks the
// instantiation by  ctc | lm << 1 | ctx << 2  from a table whose slot 0 is empty.  Nothing else in this file branches on the form.
#include <type_traits>

#include "aed_search_state.h"
#include "kernels.h"

namespace m3 {
namespace {

enum { JS_ATT = 0, JS_CTC = 1, JS_HDR = 4 };
enum { JC_TOK = 0, JC_ATT = 1, JC_CTC = 2, JC_KEY = 3, JC_WORDS = 4 };
constexpr int JT = 16;   // frames whose gathered CTC log-probabilities are in flight ahead of the serial chain
enum { LS_STATE = 0, LS_N = 1, LS_LM = 2, LS_ATT = 4, LS_WORDS = 8 };   // LM state of a row's buffer; LS_LM: a double
enum { LC_STATE = 0, LC_LM = 2, LC_WORDS = 4 };                         // LM scratch of a candidate; LC_LM: a double
// A/B switch of DESIGN.md 24: 1 = the LM walk is issued before the CTC frame chain, 0 = after it
#ifndef M3_AED_LM_WALK_FIRST
#define M3_AED_LM_WALK_FIRST 1
#endif

struct NoLm {};
struct LmFuse {
  const int32_t* image;    // the device LM image and its words
  long long words;
  const int32_t* lm_on;    // [B]
  int32_t* lstate;         // LM state: score reads buffer step & 1, prune writes the other
  int32_t* lscr;           // LM scratch: score writes, prune reads
  double alpha, beta;
  int use_eos;
};
// hotword biasing: what the CTX instantiations take besides their NoLm / LmFuse, which they inherit as they are
enum { CS_STATE = 0, CS_ATT = 1, CS_BONUS = 2, CS_WORDS = 4 };          // context state of a row's buffer; CS_BONUS: a double
enum { CC_STATE = 0, CC_BONUS = 2, CC_WORDS = 4 };                      // context scratch of a candidate; CC_BONUS: a double
struct CtxFuse {
  const int32_t* image;    // the device context image and its words
  long long words;
  const int32_t* graph_of; // [B]
  int32_t* cstate;         // context state: score reads buffer step & 1, prune writes the other
  int32_t* cscr;           // context scratch: score writes, prune reads
};
template <class L>
struct Biased : L {
  CtxFuse cx;
};

// max + log(exp(a - max) + exp(b - max)); -inf when both are: no -inf - -inf is ever formed.  exp(max - max) is exactly 1, so the
// sum is 1 + exp(min - max): one exponential, no branch (the chain of m3_aed_joint_score is one wave alone on its SIMD, its time is
// its instruction count).  The hardware exp2 / log2 behind __expf / __logf are good to about 1e-7 ABSOLUTE here (the argument of the
// exponential is <= 0, the logarithm's lies in [1, 2]); the result is added to a max of magnitude up to hundreds, whose last place
// is 100 times that.  A/B in DESIGN.md 23.
__device__ __forceinline__ float lae(float a, float b) {
  const float mx = fmaxf(a, b), mn = fminf(a, b);
  const float d = mx == -INFINITY ? 0.f : mn - mx;
  return mx + __logf(1.f + __expf(d));                            // mx = -inf: -inf + log 2
}

__device__ __forceinline__ float* js_row(float* js, int F, int row, int buf) {
  return js + ((size_t)row * 2 + buf) * (JS_HDR + 2 * (size_t)F);
}
// the utterance's CTC rows as the kernels may read them: m frames from row0, or none when the header does not fit the buffers
__device__ __forceinline__ int usable_frames(const int32_t* hdr, int F, int x_rows) {
  const int row0 = hdr[AS_MEM_ROW0], m = hdr[AS_MEM_LEN];
  return (row0 >= 0 && m >= 1 && m <= F && m <= x_rows - row0) ? m : 0;
}

// ---------------------------------------------------------------------------------------------------------------- reset
// one wave per utterance, after m3_aed_search_reset (whose headers it reads).  The state of the empty hypothesis: rn = -inf,
// rb[t] = x[0][blank] + .. + x[t][blank] summed left to right (a tile of 64 frames is loaded by the lanes and added up in frame
// order through the wave), psi = 0; att = 0 for slot 0 and -inf for the dead start slots.  Buffer 1 and the frames past m are 0.
__global__ __launch_bounds__(64) void aed_joint_reset_kernel(const int32_t* __restrict__ st, int N, int F, float* js,
                                                             const float* __restrict__ x, int ldx, int x_rows) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int32_t* hdr = as_header(st, u);
  const int m = usable_frames(hdr, F, x_rows), row0 = hdr[AS_MEM_ROW0];
  const int half = JS_HDR + 2 * F;
  for (int i = 0; i < N; ++i) {
    float* row = js_row(js, F, u * N + i, 0);
    for (int w = lane; w < 2 * half; w += 64) {
      const int off = w < half ? w : w - half;
      float v = 0.f;
      if (w < half) {
        if (off == JS_ATT) v = i == 0 ? 0.f : -INFINITY;
        if (off >= JS_HDR && off < JS_HDR + F && off - JS_HDR < m) v = -INFINITY;
        if (off >= JS_HDR + F && off - JS_HDR - F < m) continue;            // rb[t < m]: the scan below is its one writer
      }
      row[w] = v;
    }
  }
  float run = 0.f;
  for (int t0 = 0; t0 < m; t0 += 64) {
    const int t = t0 + lane;
    const float v = t < m ? x[(size_t)(row0 + t) * ldx] : 0.f;
    float mine = 0.f;
    const int cnt = min(64, m - t0);
    for (int j = 0; j < cnt; ++j) {
      run = run + lane_bcast_f(v, j);
      if (lane == j) mine = run;
    }
    if (t < m)
      for (int i = 0; i < N; ++i) js_row(js, F, u * N + i, 0)[JS_HDR + F + t] = mine;
  }
}

// ---------------------------------------------------------------------------------------------------------------- score
// one wave per hypothesis row.  The row's logsumexp and its K picks in the order of aed_search_prune_kernel (value descending,
// token id ascending); then lane j runs candidate j's prefix recursion over the utterance's m frames:
//     rn'[t] = lae(rn'[t-1], phi[t-1]) + x[t][c],  rb'[t] = lae(rn'[t-1], rb'[t-1]) + x[t][0],  psi' = lae(psi', phi[t-1] + x[t][c])
// with phi[t] = rb[t] when c repeats the parent's last token and lae(rn[t], rb[t]) otherwise.  The recursion is written from t = 1
// for every hypothesis length: below max(|g|, 1) the parent's entries are -inf, so those steps leave -inf, exactly as the
// contract's start at s = max(|g|, 1) does.  The parent's rn / rb are the same for all lanes: lane l of a 64-frame tile loads
// frame t0 + l - 1 and forms both phi variants once, the chain reads them as broadcasts.  The per-lane operand x[t][c_j] is a
// gather whose addresses do not depend on the chain: the loads of the NEXT JT frames are issued before the chain of the current JT.
//
// LM: the parent's LM state is the same for all lanes, so its back-off chain -- per level the checked arc_begin pair
// and the back-off weight summed above it, at most kLmMaxOrder levels -- is formed ONCE per wave from uniform loads into registers
// (lm_chain).  Lane j then walks token j down the levels (lm_walk): only the binary search's probes and the arc it finds go to
// memory, state 0 needs no search.  The terms and their order are lm_step's.  CTC = false: no scorer state, no chain, jkey = att'.
struct LmChain {
  int lo[kLmMaxOrder], hi[kLmMaxOrder], levels;
  double w[kLmMaxOrder + 1];                                      // w[l]: the back-off weights above level l; the last: above the root
};
__device__ __forceinline__ void lm_chain(const LmView& lm, int state, LmChain* c) {
  int st = state;
  double w = 0.0;
  c->levels = 0;
#pragma unroll
  for (int l = 0; l < kLmMaxOrder; ++l) {
    c->lo[l] = c->hi[l] = 0;
    c->w[l] = w;
    if (st != 0) {                                                // wave-uniform
      lm_arcs(lm, st, &c->lo[l], &c->hi[l]);
      w += (double)lm.bo_weight[st];
      const int nb = lm.bo_state[st];
      st = nb >= 0 && nb < st ? nb : 0;
      c->levels = l + 1;
    }
  }
  c->w[kLmMaxOrder] = w;                                          // past the last level w no longer moves: the root's weight
}
__device__ __forceinline__ double lm_walk(const LmView& lm, const LmChain& c, int tok, int* next) {
  int a = -1;
  double wa = 0.0;
#pragma unroll
  for (int l = 0; l < kLmMaxOrder; ++l)
    if (l < c.levels && a < 0) {
      a = lm_find(lm, c.lo[l], c.hi[l], tok);
      wa = c.w[l];
    }
  if (a >= 0) {
    *next = lm_in_range(lm.arc_next[a], lm.n_states);
    return wa + (double)lm.arc_logp[a];
  }
  return lm_step_root(lm, c.w[kLmMaxOrder], tok, next);
}
// the attention part of a row where the LM state keeps it (CTC = false)
__device__ __forceinline__ float lm_att(const NoLm&, int, int) { return 0.f; }
__device__ __forceinline__ float lm_att(const LmFuse& lx, int row, int buf) {
  return __builtin_bit_cast(float, lx.lstate[((size_t)row * 2 + buf) * LS_WORDS + LS_ATT]);
}
// (lm_state', lm') of a hypothesis in `state` with the sum `sum`, extended by tok: eos takes the state's final value and stays
__device__ __forceinline__ void lm_extend(const LmView& lm, int state, double sum, int tok, int eos, int use_eos, int* next,
                                          double* out) {
  const int st0 = __builtin_amdgcn_readfirstlane(lm_in_range(state, lm.n_states));
  if (tok == eos) {
    *next = st0;
    *out = sum + (double)lm.fin[st0] * (double)use_eos;
    return;
  }
  LmChain ch;
  lm_chain(lm, st0, &ch);
  *out = sum + lm_walk(lm, ch, tok, next);
}

// CTX: the attention part of a row of the <false, false, true> form, which the context state keeps
__device__ __forceinline__ float ctx_att(const CtxFuse& cx, int row, int buf) {
  return __builtin_bit_cast(float, cx.cstate[((size_t)row * 2 + buf) * CS_WORDS + CS_ATT]);
}
// (ctx_state', bonus') of a hypothesis in `state` with the credit `bonus`, extended by tok.  `state` is the same for the whole wave
// and is made uniform, so every lane gathers from ONE row of next / delta: cls[tok], then delta[state A + col] and next[state A + col].
// eos is never walked: it hands back pot[state], the credit of a phrase the hypothesis did not complete, and ends in state 0.
// No address is formed from an unchecked word: a stored state or a next entry outside [0, n_states) reads as state 0, a token
// outside [0, V) or a cls entry outside [0, A) as column 0.
__device__ __forceinline__ void ctx_extend(const CtxGraph& g, int state, double bonus, int tok, int eos, int* next, double* out) {
  const int st0 = __builtin_amdgcn_readfirstlane(state >= 0 && state < g.n_states ? state : 0);
  if (tok == eos) {
    *next = 0;
    *out = bonus - (double)g.pot[st0];
    return;
  }
  int col = tok >= 0 && tok < g.V ? g.cls[tok] : 0;
  col = col >= 0 && col < g.A ? col : 0;
  const size_t arc = (size_t)st0 * g.A + col;
  const int nx = g.next[arc];
  *out = bonus + (double)g.delta[arc];
  *next = nx >= 0 && nx < g.n_states ? nx : 0;
}

// the attention part a row starts from: the scorer state's, else the LM state's, else (CTX alone) the context state's
template <bool CTC, bool LM, bool CTX, class Lx>
__device__ __forceinline__ float row_att(const float* jr, const Lx& lx, int row, int buf) {
  if constexpr (CTX && !CTC && !LM) return ctx_att(lx.cx, row, buf);
  else return CTC ? jr[JS_ATT] : lm_att(lx, row, buf);
}

template <bool CTC, bool LM, bool CTX, class Lx>
__global__ __launch_bounds__(64) void aed_joint_score_kernel(const int32_t* __restrict__ st, int B, int N, int P, int rec_words, int V,
                                                             int K, int F, const float* __restrict__ js, int32_t* __restrict__ cand,
                                                             float* __restrict__ scr, const float* __restrict__ logits, int ldl,
                                                             const float* __restrict__ x, int ldx, int x_rows, float lam, Lx lx) {
  const int r = blockIdx.x, u = r / N, lane = threadIdx.x;
  const int32_t* hdr = as_header(st, u);
  const int s = hdr[AS_STEP];
  if (hdr[AS_DONE] != 0 || s < 0 || s >= P - 1) return;           // frozen: the scratch keeps what the last live step left
  const int eos = V - 1;
  const int32_t* rec = as_record(st, B, rec_words, r, s & 1);
  const float* jr = CTC ? js_row(const_cast<float*>(js), F, r, s & 1) : nullptr;
  const float att = row_att<CTC, LM, CTX>(jr, lx, r, s & 1), psi = CTC ? jr[JS_CTC] : 0.f;
  int32_t* crow = cand + ((size_t)r * K + lane) * JC_WORDS;       // lane j's candidate record (lanes below K)
  // LM only: the parent's (state, n, sum) as stored, lane j's scratch entry, and whether this utterance is fused at all
  [[maybe_unused]] int l_state = 0, l_n = 0;
  [[maybe_unused]] double l_sum = 0.0;
  [[maybe_unused]] int32_t* lc = nullptr;
  [[maybe_unused]] bool fused = false;
  [[maybe_unused]] LmView lm{};
  [[maybe_unused]] double l_alpha = 0.0;                          // the utterance's LM weight: a set member's scale is folded in here, once
  if constexpr (LM) {
    const int32_t* lrow = lx.lstate + ((size_t)r * 2 + (s & 1)) * LS_WORDS;
    l_state = lrow[LS_STATE];
    l_n = lrow[LS_N];
    l_sum = *reinterpret_cast<const double*>(lrow + LS_LM);
    lc = lx.lscr + ((size_t)r * K + lane) * LC_WORDS;
    l_alpha = lx.alpha;
    fused = lm_select(lx.image, lx.words, lx.lm_on[u], &lm, &l_alpha) && lm.V == V;   // uniform; a set: the utterance's member
  }
  // CTX only: the parent's (ctx_state, bonus) as stored, lane j's scratch entry, and the utterance's graph (one view per wave)
  [[maybe_unused]] int c_state = 0;
  [[maybe_unused]] double c_bonus = 0.0;
  [[maybe_unused]] int32_t* cc = nullptr;
  [[maybe_unused]] bool biased = false;
  [[maybe_unused]] CtxGraph cg{};
  if constexpr (CTX) {
    const int32_t* cs = lx.cx.cstate + ((size_t)r * 2 + (s & 1)) * CS_WORDS;
    c_state = cs[CS_STATE];
    c_bonus = *reinterpret_cast<const double*>(cs + CS_BONUS);
    cc = lx.cx.cscr + ((size_t)r * K + lane) * CC_WORDS;
    biased = ctx_graph_view(lx.cx.image, lx.cx.words, lx.cx.graph_of[u], &cg) && cg.V == V;   // uniform
  }
  if (rec[AS_FINISHED] != 0) {                                    // one candidate: increment 0, eos, the parts as they are
    if (lane < K) {
      crow[JC_TOK] = eos;
      crow[JC_ATT] = __builtin_bit_cast(int32_t, lane == 0 ? att : -INFINITY);
      crow[JC_CTC] = __builtin_bit_cast(int32_t, lane == 0 ? psi : -INFINITY);
      crow[JC_KEY] = lane == 0 ? rec[AS_SCORE] : __builtin_bit_cast(int32_t, NAN);
      if constexpr (LM) {                                         // ... and (lm_state, lm) as they are
        lc[LC_STATE] = lane == 0 ? l_state : 0;
        lc[LC_STATE + 1] = 0;
        *reinterpret_cast<double*>(lc + LC_LM) = lane == 0 ? l_sum : 0.0;
      }
      if constexpr (CTX) {                                        // ... and (ctx_state, bonus) as they are
        cc[CC_STATE] = lane == 0 ? c_state : 0;
        cc[CC_STATE + 1] = 0;
        *reinterpret_cast<double*>(cc + CC_BONUS) = lane == 0 ? c_bonus : 0.0;
      }
    }
    return;
  }
  const float* lg = logits + (size_t)r * ldl;
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, lg[c]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < V; c += 64) sum += expf(lg[c] - mx);
  const float lse = logf(wave_sum(sum));
  float pv = 0.f, my_lp = -INFINITY;
  int pi = -1, my_tok = -1;
  for (int k = 0; k < K; ++k) {
    float bv;
    int bi;
    wave_next_best(lg, V, k == 0, pv, pi, lane, bv, bi);
    if (lane == k) {
      my_tok = bi;
      my_lp = (bv - mx) - lse;
    }
    pv = bv;
    pi = bi;
    if (bi < 0) pv = -INFINITY, pi = INT_MAX;                     // nothing left (NaN logits): no further candidate
  }
  const bool is_cand = lane < K && my_tok >= 0;
  // LM: candidate j's step from the parent's state.  eos takes the state's final value and stays; an utterance that is not fused
  // carries (state, sum) along as they are
  [[maybe_unused]] int l_next = l_state;
  [[maybe_unused]] double l_new = l_sum;
  if constexpr (LM && (M3_AED_LM_WALK_FIRST || !CTC))
    if (fused) lm_extend(lm, l_state, l_sum, is_cand ? my_tok : eos, eos, lx.use_eos, &l_next, &l_new);   // idle lanes: no walk
  // CTX: candidate j's arc from the parent's state, where the LM walk sits: ahead of the frame chain, whose time covers the two
  // dependent gathers.  An utterance that is not biased carries (state, bonus) along as they are; idle lanes take no arc
  [[maybe_unused]] int c_next = c_state;
  [[maybe_unused]] double c_new = c_bonus;
  if constexpr (CTX)
    if (biased && is_cand) ctx_extend(cg, c_state, c_bonus, my_tok, eos, &c_next, &c_new);
  const int m = CTC ? usable_frames(hdr, F, x_rows) : 0, row0 = hdr[AS_MEM_ROW0];   // CTC = false: no frame, no chain
  const int last = s > 0 ? rec[AS_TOKENS + s] : -1;
  const int c = is_cand ? my_tok : 0;                             // idle lanes walk column 0: in bounds, their results unused
  const bool dead = c == 0;                                       // blank: psi' = -inf and an all -inf state
  const bool rep = c == last;
  const float* xc = x + (size_t)row0 * ldx + c;                   // formed from row0 only when m > 0 says it is in range
  const float* jrn = jr + JS_HDR;
  const float* jrb = jr + JS_HDR + F;
  float* srow = scr + (size_t)B * N * K * JC_WORDS + (size_t)r * F * 2 * K + lane;   // + (t * 2 + {0, 1}) * K

  float rn = -INFINITY, rb = -INFINITY, ps = CTC ? -INFINITY : 0.f;
  if (m > 0) {
    if (s == 0) rn = xc[0];
    ps = rn;
    if (lane < K) {
      srow[0] = dead ? -INFINITY : rn;
      srow[K] = -INFINITY;
    }
    float xg[JT], phi_a = -INFINITY, phi_b = -INFINITY, xb = 0.f;
#pragma unroll
    for (int i = 0; i < JT; ++i) xg[i] = i < m ? xc[(size_t)i * ldx] : 0.f;
    for (int t0 = 0; t0 < m; t0 += JT) {
      if ((t0 & 63) == 0) {                                       // a new 64-frame tile of the parent's state and of the blank column
        const int tp = t0 + lane - 1, tb = t0 + lane;
        const bool have = tp >= 0 && tp < m;
        const float prn = have ? jrn[tp] : -INFINITY, prb = have ? jrb[tp] : -INFINITY;
        phi_a = lae(prn, prb);
        phi_b = prb;
        xb = tb < m ? x[(size_t)(row0 + tb) * ldx] : 0.f;
      }
      float xn[JT];
#pragma unroll
      for (int i = 0; i < JT; ++i) xn[i] = t0 + JT + i < m ? xc[(size_t)(t0 + JT + i) * ldx] : 0.f;
#pragma unroll
      for (int i = 0; i < JT; ++i) {
        const int t = t0 + i;
        if (t >= 1 && t < m) {                                    // wave-uniform
          const int j = t & 63;
          const float pa = lane_bcast_f(phi_a, j), pb = lane_bcast_f(phi_b, j), xbt = lane_bcast_f(xb, j);
          const float phi = rep ? pb : pa;
          const float rn_new = lae(rn, phi) + xg[i];
          rb = lae(rn, rb) + xbt;
          ps = lae(ps, phi + xg[i]);
          rn = rn_new;
          if (lane < K) {
            srow[(size_t)t * 2 * K] = dead ? -INFINITY : rn;
            srow[(size_t)t * 2 * K + K] = dead ? -INFINITY : rb;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < JT; ++i) xg[i] = xn[i];
    }
    if (c == eos) ps = lae(jrn[m - 1], jrb[m - 1]);
  }
  if (CTC && dead) ps = -INFINITY;
  if constexpr (LM && CTC && !M3_AED_LM_WALK_FIRST)
    if (fused) lm_extend(lm, l_state, l_sum, is_cand ? my_tok : eos, eos, lx.use_eos, &l_next, &l_new);
  if (lane < K) {
    const float att2 = att + my_lp;                               // -inf + increment stays -inf
    float key = NAN;
    if constexpr (CTC) {
      if (is_cand) key = (att2 == -INFINITY || ps == -INFINITY) ? -INFINITY : (1.f - lam) * att2 + lam * ps;
    } else {
      if (is_cand) key = att2;
    }
    if constexpr (LM) {                                           // two products and one sum in double, rounded once
      if constexpr (!CTX)
        if (fused && is_cand && key != -INFINITY) key = key + (float)(l_alpha * l_new + lx.beta * (double)(l_n + 1));
      lc[LC_STATE] = is_cand ? l_next : 0;
      lc[LC_STATE + 1] = 0;
      *reinterpret_cast<double*>(lc + LC_LM) = is_cand ? l_new : 0.0;
    }
    if constexpr (CTX) {                                          // extra = (alpha lm' + beta n') + bonus' in double, rounded once
      if (is_cand && key != -INFINITY) {
        if constexpr (LM) {
          if (fused && biased) key = key + (float)((l_alpha * l_new + lx.beta * (double)(l_n + 1)) + c_new);
          else if (fused) key = key + (float)(l_alpha * l_new + lx.beta * (double)(l_n + 1));
          else if (biased) key = key + (float)c_new;
        } else {
          if (biased) key = key + (float)c_new;
        }
      }
      cc[CC_STATE] = is_cand ? c_next : 0;
      cc[CC_STATE + 1] = 0;
      *reinterpret_cast<double*>(cc + CC_BONUS) = is_cand ? c_new : 0.0;
    }
    crow[JC_TOK] = is_cand ? my_tok : eos;
    crow[JC_ATT] = __builtin_bit_cast(int32_t, is_cand ? att2 : -INFINITY);
    crow[JC_CTC] = __builtin_bit_cast(int32_t, is_cand ? ps : -INFINITY);
    crow[JC_KEY] = __builtin_bit_cast(int32_t, key);
  }
}

// ---------------------------------------------------------------------------------------------------------------- prune
// one work-group per utterance: wave 0 picks the N largest of the N * K keys (ties to the lower flat index row * K + rank; a
// NaN key is no candidate), all threads copy the parents' token and ancestry paths into the other record exactly as
// aed_search_prune_kernel does and the survivors' scorer states from the scratch into the other buffer, thread 0 moves the step.
// LM: a survivor's (lm_state, lm) is copied from the LM scratch, its n is the parent's plus one unless the parent was finished.
template <bool CTC, bool LM, bool CTX, class Lx>
__global__ __launch_bounds__(256) void aed_joint_prune_kernel(int32_t* st, int B, int N, int P, int rec_words, int V, int K, int F,
                                                              float* js, const int32_t* __restrict__ cand,
                                                              const float* __restrict__ scr, int32_t* __restrict__ done_out, Lx lx) {
  __shared__ float c_key[AS_MAX_BEAM * AS_MAX_BEAM];
  __shared__ int32_t pick[AS_MAX_BEAM];
  const int u = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int32_t* hdr = as_header(st, u);
  const int s = hdr[AS_STEP], limit = hdr[AS_LIMIT];
  if (hdr[AS_DONE] != 0 || s < 0 || s >= P - 1) {                  // frozen: not one word of the utterance changes
    if (tid == 0 && done_out) done_out[u] = 1;
    return;
  }
  [[maybe_unused]] const int m = (hdr[AS_MEM_LEN] >= 1 && hdr[AS_MEM_LEN] <= F) ? hdr[AS_MEM_LEN] : 0;   // only t < F is ever addressed
  const int cur = s & 1, nxt = cur ^ 1, eos = V - 1;
  const int32_t* ucand = cand + (size_t)u * N * K * JC_WORDS;
  for (int idx = tid; idx < N * K; idx += 256) c_key[idx] = __builtin_bit_cast(float, ucand[(size_t)idx * JC_WORDS + JC_KEY]);
  __syncthreads();
  if (w == 0) {
    float pv = 0.f;
    int pi = -1;
    for (int j = 0; j < N; ++j) {
      float bv;
      int bi;
      wave_next_best(c_key, N * K, j == 0, pv, pi, lane, bv, bi);
      if (lane == 0) pick[j] = bi;
      pv = bv;
      pi = bi;
      if (bi < 0) pv = -INFINITY, pi = INT_MAX;
    }
  }
  __syncthreads();
  const int span = s + 1;
  for (int idx = tid; idx < N * span; idx += 256) {
    const int j = idx / span, t = idx - j * span;
    const int parent = pick[j] >= 0 ? pick[j] / K : 0;
    const int32_t* src = as_record(st, B, rec_words, u * N + parent, cur);
    int32_t* dst = const_cast<int32_t*>(as_record(st, B, rec_words, u * N + j, nxt));
    dst[AS_TOKENS + t] = src[AS_TOKENS + t];
    dst[AS_TOKENS + P + t] = t < s ? src[AS_TOKENS + P + t] : parent;
  }
  if constexpr (CTC)
    for (int idx = tid; idx < N * m; idx += 256) {                // the states of the survivors that can be extended again
      const int j = idx / m, t = idx - j * m, c = pick[j];
      if (c < 0 || ucand[(size_t)c * JC_WORDS + JC_TOK] == eos) continue;
      const int parent = c / K, rank = c - parent * K;
      const float* src = scr + (size_t)B * N * K * JC_WORDS + ((size_t)(u * N + parent) * F + t) * 2 * K + rank;
      float* dst = js_row(js, F, u * N + j, nxt) + JS_HDR;
      dst[t] = src[0];
      dst[F + t] = src[K];
    }
  if (tid < N) {
    const int j = tid, c = pick[j];
    const int32_t* cr = ucand + (size_t)(c >= 0 ? c : 0) * JC_WORDS;
    const int tok = c >= 0 ? cr[JC_TOK] : eos;
    int32_t* dst = const_cast<int32_t*>(as_record(st, B, rec_words, u * N + j, nxt));
    dst[AS_SCORE] = c >= 0 ? cr[JC_KEY] : __builtin_bit_cast(int32_t, -INFINITY);
    dst[AS_FINISHED] = tok == eos;
    dst[AS_TOKENS + s + 1] = tok;
    if constexpr (CTC) {
      int32_t* jd = reinterpret_cast<int32_t*>(js_row(js, F, u * N + j, nxt));
      jd[JS_ATT] = c >= 0 ? cr[JC_ATT] : __builtin_bit_cast(int32_t, -INFINITY);
      jd[JS_CTC] = c >= 0 ? cr[JC_CTC] : __builtin_bit_cast(int32_t, -INFINITY);
    }
    if constexpr (LM) {
      const int parent = c >= 0 ? c / K : 0;
      const int32_t* lp = lx.lstate + ((size_t)(u * N + parent) * 2 + cur) * LS_WORDS;
      const int32_t* lcs = lx.lscr + ((size_t)u * N * K + (c >= 0 ? c : 0)) * LC_WORDS;
      const bool grew = as_record(st, B, rec_words, u * N + parent, cur)[AS_FINISHED] == 0;
      int32_t* ld = lx.lstate + ((size_t)(u * N + j) * 2 + nxt) * LS_WORDS;
      ld[LS_STATE] = c >= 0 ? lcs[LC_STATE] : 0;
      ld[LS_N] = c >= 0 ? lp[LS_N] + (grew ? 1 : 0) : 0;
      *reinterpret_cast<double*>(ld + LS_LM) = c >= 0 ? *reinterpret_cast<const double*>(lcs + LC_LM) : 0.0;
      ld[LS_ATT] = CTC ? 0 : (c >= 0 ? cr[JC_ATT] : __builtin_bit_cast(int32_t, -INFINITY));
    }
    if constexpr (CTX) {                                          // the survivor's (ctx_state', bonus') as score left them
      const int32_t* ccs = lx.cx.cscr + ((size_t)u * N * K + (c >= 0 ? c : 0)) * CC_WORDS;
      int32_t* cd = lx.cx.cstate + ((size_t)(u * N + j) * 2 + nxt) * CS_WORDS;
      cd[CS_STATE] = c >= 0 ? ccs[CC_STATE] : 0;
      cd[CS_ATT] = (CTC || LM) ? 0 : (c >= 0 ? cr[JC_ATT] : __builtin_bit_cast(int32_t, -INFINITY));
      *reinterpret_cast<double*>(cd + CS_BONUS) = c >= 0 ? *reinterpret_cast<const double*>(ccs + CC_BONUS) : 0.0;
    }
  }
  if (tid == 0) {
    bool all = true;
    for (int j = 0; j < N; ++j) all = all && (pick[j] < 0 || ucand[(size_t)pick[j] * JC_WORDS + JC_TOK] == eos);
    const int done = all || s + 1 >= limit;
    int32_t* h = const_cast<int32_t*>(hdr);
    h[AS_STEP] = s + 1;                                           // every thread read the header before the first barrier
    h[AS_DONE] = done;
    if (done_out) done_out[u] = done;
  }
}

// --------------------------------------------------------------------------------------------------------------- result
__global__ __launch_bounds__(64) void aed_joint_result_kernel(const int32_t* __restrict__ st, int N, int P, int F,
                                                              const float* __restrict__ js, float* __restrict__ att,
                                                              float* __restrict__ ctc) {
  const int u = blockIdx.x, j = threadIdx.x;
  const int s = min(max(as_header(st, u)[AS_STEP], 0), P - 1);
  if (j < N) {
    const float* jr = js_row(const_cast<float*>(js), F, u * N + j, s & 1);
    att[u * N + j] = jr[JS_ATT];
    ctc[u * N + j] = jr[JS_CTC];
  }
}

// ------------------------------------------------------------------------------------------------------------------- LM
// one thread per row, after m3_aed_search_reset: [sos] is in the image's start state with sum 0.0 and n = 0; buffer 1 is 0
__global__ __launch_bounds__(256) void aed_lm_reset_kernel(int R, int N, int32_t* ls, int start) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  int32_t* row = ls + (size_t)r * 2 * LS_WORDS;
  for (int w = 0; w < 2 * LS_WORDS; ++w) row[w] = 0;
  row[LS_STATE] = start;
  row[LS_ATT] = __builtin_bit_cast(int32_t, r % N == 0 ? 0.f : -INFINITY);
}

// the same with the start state of each utterance's own LM: the member lm_on picks from a set (or the single image, lm_on != 0);
// an utterance that runs without the LM holds state 0
__global__ __launch_bounds__(256) void aed_lm_reset_set_kernel(int R, int N, int V, int32_t* ls, const int32_t* __restrict__ image,
                                                               long long words, const int32_t* __restrict__ lm_on) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  LmView lm;
  double alpha = 0.0;
  const bool fused = lm_select(image, words, lm_on[r / N], &lm, &alpha) && lm.V == V;
  int32_t* row = ls + (size_t)r * 2 * LS_WORDS;
  for (int w = 0; w < 2 * LS_WORDS; ++w) row[w] = 0;
  row[LS_STATE] = fused ? lm.start : 0;
  row[LS_ATT] = __builtin_bit_cast(int32_t, r % N == 0 ? 0.f : -INFINITY);
}

__global__ __launch_bounds__(64) void aed_lm_result_kernel(const int32_t* __restrict__ st, int N, int P, const int32_t* __restrict__ ls,
                                                           float* __restrict__ lm, int32_t* __restrict__ lm_state, int32_t* __restrict__ n,
                                                           float* __restrict__ att) {
  const int u = blockIdx.x, j = threadIdx.x;
  const int s = min(max(as_header(st, u)[AS_STEP], 0), P - 1);
  if (j < N) {
    const int32_t* row = ls + ((size_t)(u * N + j) * 2 + (s & 1)) * LS_WORDS;
    lm[u * N + j] = (float)*reinterpret_cast<const double*>(row + LS_LM);
    lm_state[u * N + j] = row[LS_STATE];
    if (n) n[u * N + j] = row[LS_N];
    if (att) att[u * N + j] = __builtin_bit_cast(float, row[LS_ATT]);
  }
}

// -------------------------------------------------------------------------------------------------------------- context
// one thread per row, after m3_aed_search_reset: [sos] is in state 0 with bonus 0.0; buffer 1 is 0
__global__ __launch_bounds__(256) void aed_bias_reset_kernel(int R, int N, int32_t* cs) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  int32_t* row = cs + (size_t)r * 2 * CS_WORDS;
  for (int w = 0; w < 2 * CS_WORDS; ++w) row[w] = 0;
  row[CS_ATT] = __builtin_bit_cast(int32_t, r % N == 0 ? 0.f : -INFINITY);
}

__global__ __launch_bounds__(64) void aed_bias_result_kernel(const int32_t* __restrict__ st, int N, int P, const int32_t* __restrict__ cs,
                                                             float* __restrict__ bonus, int32_t* __restrict__ ctx_state,
                                                             float* __restrict__ att) {
  const int u = blockIdx.x, j = threadIdx.x;
  const int s = min(max(as_header(st, u)[AS_STEP], 0), P - 1);
  if (j < N) {
    const int32_t* row = cs + ((size_t)(u * N + j) * 2 + (s & 1)) * CS_WORDS;
    bonus[u * N + j] = (float)*reinterpret_cast<const double*>(row + CS_BONUS);
    ctx_state[u * N + j] = row[CS_STATE];
    if (att) att[u * N + j] = __builtin_bit_cast(float, row[CS_ATT]);
  }
}

// ------------------------------------------------------------------------------------------------------- the host half
//   Every entry point fills a FusedCall, states the pre-conditions that are its own, and hands it to check_call and,
// for the two kernel templates, to launch_fused.  Nothing below knows which family it was called through beyond FusedCall::family.
size_t rows_of(const m3_aed_joint_desc* d) { return (size_t)d->search.B * d->search.beam; }
size_t joint_state_bytes(const m3_aed_joint_desc* d) { return align_up(4 * rows_of(d) * 2 * (JS_HDR + 2 * (size_t)d->max_frames), 256); }
size_t joint_scratch_bytes(const m3_aed_joint_desc* d) {
  return align_up(4 * rows_of(d) * d->pre_beam * (JC_WORDS + 2 * (size_t)d->max_frames), 256);
}
size_t lm_state_bytes(const m3_aed_joint_desc* d) { return align_up(4 * rows_of(d) * 2 * LS_WORDS, 256); }
size_t lm_scratch_bytes(const m3_aed_joint_desc* d) { return align_up(4 * rows_of(d) * d->pre_beam * (LC_WORDS + JC_WORDS), 256); }
size_t bias_state_bytes(const m3_aed_joint_desc* d) { return align_up(4 * rows_of(d) * 2 * CS_WORDS, 256); }
size_t bias_scratch_bytes(const m3_aed_joint_desc* d) { return align_up(4 * rows_of(d) * d->pre_beam * (CC_WORDS + JC_WORDS), 256); }

enum Family { JOINT = 0, NGRAM = 1, BIAS = 2 };                   // the entry point's family: each asks what the one before it asks
const char* const kFamily[] = {"aed_joint", "aed_ngram", "aed_bias"};

// What a descriptor must hold.  The search's own checks; V and the pre-beam; with CTC the frames and the int32 offsets of the
// scorer state and the joint scratch (without it there is no scorer state and max_frames is not looked at); from the LM family on
// the offsets of the two LM blobs, in the bias family those of the two context blobs.  A rule speaks as the family that brought it.
int check_desc(const m3_aed_joint_desc* d, Family family, bool ctc) {
  M3_REQUIRE(d != nullptr, "%s: null descriptor", kFamily[family]);
  if (int rc = check_search_desc(&d->search)) return rc;
  const m3_aed_search_desc* s = &d->search;
  const char* who = kFamily[ctc ? JOINT : NGRAM];
  M3_REQUIRE(s->V >= 2, "%s: V = %d, %s and eos need two different ids", who, s->V, ctc ? "blank" : "a token");
  M3_REQUIRE(d->pre_beam >= s->beam && d->pre_beam <= AS_MAX_BEAM && d->pre_beam <= s->V,
             "%s: pre_beam = %d, need beam = %d <= pre_beam <= min(%d, V = %d)", who, d->pre_beam, s->beam, AS_MAX_BEAM, s->V);
  const size_t R = rows_of(d), K = (size_t)d->pre_beam;
  if (ctc) {
    M3_REQUIRE(d->max_frames >= 1 && d->max_frames <= (1 << 20), "aed_joint: max_frames = %d outside [1, 2^20]", d->max_frames);
    const size_t F = (size_t)d->max_frames;
    M3_REQUIRE(R * 2 * (JS_HDR + 2 * F) <= (size_t)INT_MAX, "aed_joint: %zu rows of %zu frames overflow the int32 offsets of the scorer state", R, F);
    M3_REQUIRE(R * K * (JC_WORDS + 2 * F) <= (size_t)INT_MAX,
               "aed_joint: %zu rows x %zu candidates x %zu frames overflow the int32 offsets of the candidate scratch", R, K, F);
  }
  if (family >= NGRAM) {
    M3_REQUIRE(R * 2 * LS_WORDS <= (size_t)INT_MAX, "aed_ngram: %zu rows overflow the int32 offsets of the LM state", R);
    M3_REQUIRE(R * K * (LC_WORDS + JC_WORDS) <= (size_t)INT_MAX, "aed_ngram: %zu rows x %zu candidates overflow the int32 offsets of the LM scratch", R, K);
  }
  if (family == BIAS) {
    M3_REQUIRE(R * 2 * CS_WORDS <= (size_t)INT_MAX, "aed_bias: %zu rows overflow the int32 offsets of the context state", R);
    M3_REQUIRE(R * K * (CC_WORDS + JC_WORDS) <= (size_t)INT_MAX, "aed_bias: %zu rows x %zu candidates overflow the int32 offsets of the context scratch", R, K);
  }
  return 0;
}

// a blob of a call: at least `need` bytes, non-null unless the batch is empty, 16-byte aligned
int check_blob(const char* what, const char* noun, const void* p, size_t bytes, size_t need, int B) {
  M3_REQUIRE(bytes >= need, "%s: %s %zu bytes < required %zu", what, noun, bytes, need);
  M3_REQUIRE(B == 0 || (p != nullptr && ((uintptr_t)p & 15) == 0), "%s: the %s must be 16-byte aligned device memory", what, noun);
  return 0;
}

// the bias record of an entry point: the image (where the call reads it), graph_of, the context state and (with_scratch) scratch
int check_bias(const m3_aed_joint_desc* d, const m3_aed_bias* b, bool with_image, bool with_scratch, const char* what) {
  M3_REQUIRE(b != nullptr, "%s: null bias record", what);
  const int B = d->search.B;
  if (with_image) {
    M3_REQUIRE(b->image_bytes % 4 == 0 && b->image_bytes >= CTX_HDR_WORDS * 4 && b->image_bytes <= kCtxMaxBytes && b->image != nullptr,
               "%s: context image of %zu bytes (a multiple of 4 in [%d, %zu])", what, b->image_bytes, CTX_HDR_WORDS * 4, kCtxMaxBytes);
    M3_REQUIRE(B == 0 || b->graph_of != nullptr, "%s: null graph_of", what);
  }
  if (int rc = check_blob(what, "context state", b->state, b->state_bytes, bias_state_bytes(d), B)) return rc;
  return with_scratch ? check_blob(what, "context scratch", b->scratch, b->scratch_bytes, bias_scratch_bytes(d), B) : 0;
}

// Everything a score / prune / result / reset entry point receives.  ctc, lm and ctx say which parts this call has; the members of
// a part the call does not have, and the inputs an entry point does not take (prune has no image and no weights), stay zero.
// The blobs are const here whoever writes them: the launch casts, as the entry points did.
struct FusedCall {
  const char* what;                              // the entry point's name, for the messages
  Family family;
  bool ctc, lm, ctx;
  const m3_aed_joint_desc* d;
  const void* st;                                // search state
  size_t st_bytes;
  const void *js, *scr;                          // CTC: scorer state, joint scratch; the log-probabilities and ctc_weight
  size_t js_bytes, scr_bytes;
  const float* x;
  int ldx, x_rows;
  float lam;
  const void *ls, *lscr;                         // LM: state, scratch; the image, lm_on and the weights
  size_t ls_bytes, lscr_bytes;
  const void* image;
  size_t image_bytes;
  const int32_t* lm_on;
  double alpha, beta;
  int use_eos;
  const m3_aed_bias* bias;                       // context: the caller's record
  const float* logits;
  int ldl;
  int32_t* done;
  hipStream_t stream;
  bool empty() const { return d != nullptr && d->search.B == 0; }
};
// what every entry point has; the rest zero
FusedCall fused_call(const char* what, Family family, bool ctc, bool lm, bool ctx, const m3_aed_joint_desc* d, const void* st, size_t st_bytes,
                     m3_stream stream) {
  FusedCall c{};
  c.what = what, c.family = family, c.ctc = ctc, c.lm = lm, c.ctx = ctx, c.d = d, c.st = st, c.st_bytes = st_bytes, c.stream = (hipStream_t)stream;
  return c;
}

// Everything an entry point checks about its descriptor and its blobs, in this order: the descriptor; no LM blob without an LM;
// the search state; with CTC the scorer state; with an LM the LM state; with a context the caller's record.  with_scratch: the
// scratch blobs are part of this call (score and prune); with_image: so is the context image (score).
int check_call(const FusedCall& c, bool with_scratch, bool with_image) {
  const m3_aed_joint_desc* d = c.d;
  if (int rc = check_desc(d, c.family, c.ctc)) return rc;
  const int B = d->search.B;
  if (!c.lm) M3_REQUIRE(c.ls == nullptr && c.lscr == nullptr, "%s: an LM blob without the other (LM state and LM scratch are NULL exactly when there is no LM)", c.what);
  if (int rc = check_search_state(&d->search, c.st, c.st_bytes, c.what)) return rc;
  if (c.ctc) {
    if (int rc = check_blob(c.what, "scorer state", c.js, c.js_bytes, joint_state_bytes(d), B)) return rc;
    if (with_scratch)
      if (int rc = check_blob(c.what, "scratch", c.scr, c.scr_bytes, joint_scratch_bytes(d), B)) return rc;
  }
  if (c.lm) {
    if (int rc = check_blob(c.what, "LM state", c.ls, c.ls_bytes, lm_state_bytes(d), B)) return rc;
    if (with_scratch)
      if (int rc = check_blob(c.what, "LM scratch", c.lscr, c.lscr_bytes, lm_scratch_bytes(d), B)) return rc;
  }
  return c.ctx ? check_bias(d, c.bias, with_image, with_scratch, c.what) : 0;
}

int check_ctc(const FusedCall& c) {
  M3_REQUIRE(c.ldx >= c.d->search.V, "%s: ldc = %d < V = %d", c.what, c.ldx, c.d->search.V);
  M3_REQUIRE(c.x_rows >= 0, "%s: ctc_rows = %d", c.what, c.x_rows);
  M3_REQUIRE(c.d->search.B == 0 || c.x != nullptr, "%s: null CTC log-probabilities", c.what);
  return 0;
}

int check_lm_args(const FusedCall& c) {
  const int B = c.d->search.B;
  M3_REQUIRE(B == 0 || c.lm_on != nullptr, "%s: null lm_on", c.what);
  M3_REQUIRE(B == 0 || c.image != nullptr, "%s: null LM image", c.what);
  // a single image or a set: which one only the device copy says, so the bound is the set's
  M3_REQUIRE(c.image_bytes % 4 == 0 && c.image_bytes >= LM_HDR_WORDS * 4 && c.image_bytes <= kLmSetMaxBytes,
             "%s: LM image of %zu bytes (a multiple of 4 in [%d, %zu])", c.what, c.image_bytes, LM_HDR_WORDS * 4, kLmSetMaxBytes);
  return 0;
}

// ---- the launch table: THE launch of each kernel template, and the form's index  ctc | lm << 1 | ctx << 2  into eight pointers.
// What a form passes follows from its flags alone.  Lx: NoLm or LmFuse, inside Biased<> with a context.  The candidate records:
// the joint scratch with CTC, else behind the LM scratch's (state, sum) pairs, else behind the context scratch's (state, bonus)
// pairs.  Without CTC there is no scorer state and no frame: F, js, scr, x, ldx, x_rows and lam are zero.  score: the launch reads
// the context image and graph_of (prune gets the state and scratch pointers alone; its LM inputs are zero in the record already).
template <bool LM, bool CTX>
auto make_lx(const FusedCall& c, bool score) {
  std::conditional_t<LM, LmFuse, NoLm> l{};
  if constexpr (LM)
    l = LmFuse{(const int32_t*)c.image, (long long)(c.image_bytes / 4), c.lm_on, (int32_t*)c.ls, (int32_t*)c.lscr, c.alpha, c.beta, c.use_eos};
  if constexpr (CTX) {
    const m3_aed_bias* b = c.bias;
    const CtxFuse cx{score ? (const int32_t*)b->image : nullptr, score ? (long long)(b->image_bytes / 4) : 0, score ? b->graph_of : nullptr,
                     (int32_t*)b->state, (int32_t*)b->scratch};
    return Biased<decltype(l)>{l, cx};
  } else {
    return l;
  }
}
template <bool CTC, bool LM>
int32_t* cand_of(const FusedCall& c) {
  const size_t RK = rows_of(c.d) * c.d->pre_beam;
  if (CTC) return (int32_t*)c.scr;
  return LM ? (int32_t*)c.lscr + RK * LC_WORDS : (int32_t*)c.bias->scratch + RK * CC_WORDS;
}

template <bool CTC, bool LM, bool CTX>
void launch_score(const FusedCall& c) {
  const m3_aed_search_desc* s = &c.d->search;
  const SearchLayout l = search_layout(s);
  auto lx = make_lx<LM, CTX>(c, true);
  hipLaunchKernelGGL((aed_joint_score_kernel<CTC, LM, CTX, decltype(lx)>), dim3((unsigned)(s->B * s->beam)), dim3(64), 0, c.stream,
                     (const int32_t*)c.st, s->B, s->beam, l.P, l.rec_words, s->V, c.d->pre_beam, CTC ? c.d->max_frames : 0,
                     CTC ? (const float*)c.js : nullptr, cand_of<CTC, LM>(c), CTC ? (float*)c.scr : nullptr, c.logits, c.ldl,
                     CTC ? c.x : nullptr, CTC ? c.ldx : 0, CTC ? c.x_rows : 0, CTC ? c.lam : 0.f, lx);
}
template <bool CTC, bool LM, bool CTX>
void launch_prune(const FusedCall& c) {
  const m3_aed_search_desc* s = &c.d->search;
  const SearchLayout l = search_layout(s);
  auto lx = make_lx<LM, CTX>(c, false);
  hipLaunchKernelGGL((aed_joint_prune_kernel<CTC, LM, CTX, decltype(lx)>), dim3((unsigned)s->B), dim3(256), 0, c.stream, (int32_t*)c.st, s->B,
                     s->beam, l.P, l.rec_words, s->V, c.d->pre_beam, CTC ? c.d->max_frames : 0, CTC ? (float*)c.js : nullptr,
                     (const int32_t*)cand_of<CTC, LM>(c), CTC ? (const float*)c.scr : nullptr, c.done, lx);
}

// slot 0, no CTC, no LM and no context, is empty: that step is m3_aed_search_prune in aed_search.hip, and no entry point here
// can ask for it.  Reaching it is a refusal, not a launch.
using FusedLaunch = void (*)(const FusedCall&);
const FusedLaunch kScore[8] = {nullptr, launch_score<true, false, false>, launch_score<false, true, false>, launch_score<true, true, false>,
                               launch_score<false, false, true>, launch_score<true, false, true>, launch_score<false, true, true>, launch_score<true, true, true>};
const FusedLaunch kPrune[8] = {nullptr, launch_prune<true, false, false>, launch_prune<false, true, false>, launch_prune<true, true, false>,
                               launch_prune<false, false, true>, launch_prune<true, false, true>, launch_prune<false, true, true>, launch_prune<true, true, true>};

int launch_fused(const FusedLaunch (&table)[8], const FusedCall& c) {
  if (c.d->search.B == 0) return 0;
  const FusedLaunch launch = table[(int)c.ctc | (int)c.lm << 1 | (int)c.ctx << 2];
  M3_REQUIRE(launch != nullptr, "%s: a step without CTC, LM and context is m3_aed_search_prune", c.what);
  launch(c);
  M3_LAUNCH_CHECK();
  return 0;
}

// score: the blobs, then the inputs in the order CTC, logits, LM.  The weights are looked at with an LM or a context; a call with
// neither is the joint step alone, whose ctc_weight cannot be 0.
int fused_score(const FusedCall& c) {
  if (int rc = check_call(c, true, true)) return rc;
  const m3_aed_search_desc* s = &c.d->search;
  if (c.ctc)
    if (int rc = check_ctc(c)) return rc;
  M3_REQUIRE(c.ldl >= s->V, "%s: ldl = %d < V = %d", c.what, c.ldl, s->V);
  if (c.lm)
    if (int rc = check_lm_args(c)) return rc;
  if (c.lm || c.ctx)
    M3_REQUIRE(std::isfinite(c.alpha) && std::isfinite(c.beta), "%s: alpha or beta is not finite", c.what);
  else
    M3_REQUIRE(c.lam > 0.f && c.lam <= 1.f, "%s: ctc_weight = %g outside (0, 1] (0 is m3_aed_search_prune)", c.what, (double)c.lam);
  M3_REQUIRE(!c.lm || c.use_eos == 0 || c.use_eos == 1, "%s: use_eos = %d", c.what, c.use_eos);
  M3_REQUIRE(s->B == 0 || c.logits != nullptr, "%s: null pointer", c.what);
  return launch_fused(kScore, c);
}

int fused_prune(const FusedCall& c) {
  if (int rc = check_call(c, true, false)) return rc;
  return launch_fused(kPrune, c);
}

// Both m3_aed_ngram_reset entries.  set: the image may be an LM set (its bound, lm_on picks each utterance's member).  The header is
// read back once per search, a set's 8 words or a single image's 20: what is refused here the kernels would run as "LM off".
int lm_reset(const char* what, bool set, const m3_aed_joint_desc* d, void* ls, size_t ls_bytes, const void* image, size_t bytes,
             const int32_t* lm_on, m3_stream stream) {
  const size_t max_bytes = set ? kLmSetMaxBytes : kLmMaxBytes;
  if (int rc = check_desc(d, NGRAM, false)) return rc;
  if (int rc = check_blob(what, "LM state", ls, ls_bytes, lm_state_bytes(d), d->search.B)) return rc;
  M3_REQUIRE(bytes % 4 == 0 && bytes >= LM_HDR_WORDS * 4 && bytes <= max_bytes && image != nullptr, "%s: LM image of %zu bytes (a multiple of 4 in [%d, %zu])",
             what, bytes, LM_HDR_WORDS * 4, max_bytes);
  M3_REQUIRE(!set || d->search.B == 0 || lm_on != nullptr, "%s: null lm_on", what);
  int32_t head[LM_HDR_WORDS];
  M3_CHECK_HIP(hipMemcpy(head, image, sizeof(head), hipMemcpyDeviceToHost));
  const long long words = (long long)(bytes / 4);
  LmView view;
  int image_V = 0;
  if (set && lm_is_set(head, words)) {
    M3_REQUIRE(head[LMS_VERSION] == kLmSetVersion && head[LMS_G] >= 1 && head[LMS_G] <= kLmSetMaxMembers && head[LMS_WORDS] == words,
               "%s: the LM set's header (version %d, G = %d, %d words) does not describe a set of %zu bytes", what, head[LMS_VERSION], head[LMS_G],
               head[LMS_WORDS], bytes);
    image_V = head[LMS_V];
  } else {
    M3_REQUIRE(lm_view(head, words, &view), "%s: the LM image's header does not describe an image of %zu bytes", what, bytes);
    image_V = view.V;
  }
  M3_REQUIRE(image_V == d->search.V, "%s: the LM image was built for V = %d, the search has V = %d", what, image_V, d->search.V);
  if (d->search.B == 0) return 0;
  const int R = d->search.B * d->search.beam;
  if (set)
    hipLaunchKernelGGL(aed_lm_reset_set_kernel, dim3((unsigned)cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, R, d->search.beam, d->search.V,
                       (int32_t*)ls, (const int32_t*)image, words, lm_on);
  else
    hipLaunchKernelGGL(aed_lm_reset_kernel, dim3((unsigned)cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, R, d->search.beam, (int32_t*)ls, view.start);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace m3

using namespace m3;

extern "C" {

size_t m3_aed_joint_state_size(const m3_aed_joint_desc* desc) { return check_desc(desc, JOINT, true) ? 0 : joint_state_bytes(desc); }
size_t m3_aed_joint_scratch_size(const m3_aed_joint_desc* desc) { return check_desc(desc, JOINT, true) ? 0 : joint_scratch_bytes(desc); }
size_t m3_aed_ngram_state_size(const m3_aed_joint_desc* desc) { return check_desc(desc, NGRAM, false) ? 0 : lm_state_bytes(desc); }
size_t m3_aed_ngram_scratch_size(const m3_aed_joint_desc* desc) { return check_desc(desc, NGRAM, false) ? 0 : lm_scratch_bytes(desc); }
size_t m3_aed_bias_state_size(const m3_aed_joint_desc* desc) { return check_desc(desc, BIAS, false) ? 0 : bias_state_bytes(desc); }
size_t m3_aed_bias_scratch_size(const m3_aed_joint_desc* desc) { return check_desc(desc, BIAS, false) ? 0 : bias_scratch_bytes(desc); }

// ---- m3_aed_joint_*: always the CTC part, nothing else
int m3_aed_joint_reset(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, void* joint_state,
                       size_t joint_state_bytes, const float* ctc, int ldc, int ctc_rows, m3_stream stream) {
  FusedCall c = fused_call("aed_joint_reset", JOINT, true, false, false, desc, search_state, search_state_bytes, stream);
  c.js = joint_state, c.js_bytes = joint_state_bytes;
  c.x = ctc, c.ldx = ldc, c.x_rows = ctc_rows;
  if (int rc = check_call(c, false, false)) return rc;
  if (int rc = check_ctc(c)) return rc;
  if (desc->search.B == 0) return 0;
  hipLaunchKernelGGL(aed_joint_reset_kernel, dim3((unsigned)desc->search.B), dim3(64), 0, c.stream, (const int32_t*)search_state,
                     desc->search.beam, desc->max_frames, (float*)joint_state, ctc, ldc, ctc_rows);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_joint_score(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                       size_t joint_state_bytes, void* scratch, size_t scratch_bytes, const float* logits, int ldl, const float* ctc,
                       int ldc, int ctc_rows, float ctc_weight, m3_stream stream) {
  FusedCall c = fused_call("aed_joint_score", JOINT, true, false, false, desc, search_state, search_state_bytes, stream);
  c.js = joint_state, c.js_bytes = joint_state_bytes, c.scr = scratch, c.scr_bytes = scratch_bytes;
  c.x = ctc, c.ldx = ldc, c.x_rows = ctc_rows, c.lam = ctc_weight;
  c.logits = logits, c.ldl = ldl;
  return fused_score(c);
}

int m3_aed_joint_prune(const m3_aed_joint_desc* desc, void* search_state, size_t search_state_bytes, void* joint_state,
                       size_t joint_state_bytes, const void* scratch, size_t scratch_bytes, int32_t* done, m3_stream stream) {
  FusedCall c = fused_call("aed_joint_prune", JOINT, true, false, false, desc, search_state, search_state_bytes, stream);
  c.js = joint_state, c.js_bytes = joint_state_bytes, c.scr = scratch, c.scr_bytes = scratch_bytes;
  c.done = done;
  return fused_prune(c);
}

int m3_aed_joint_result(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                        size_t joint_state_bytes, float* att, float* ctc, m3_stream stream) {
  FusedCall c = fused_call("aed_joint_result", JOINT, true, false, false, desc, search_state, search_state_bytes, stream);
  c.js = joint_state, c.js_bytes = joint_state_bytes;
  if (int rc = check_call(c, false, false)) return rc;
  if (desc->search.B == 0) return 0;
  M3_REQUIRE(att && ctc, "aed_joint_result: null pointer");
  hipLaunchKernelGGL(aed_joint_result_kernel, dim3((unsigned)desc->search.B), dim3(64), 0, c.stream, (const int32_t*)search_state,
                     desc->search.beam, search_layout(&desc->search).P, desc->max_frames, (const float*)joint_state, att, ctc);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---- m3_aed_ngram_*: always the LM part; the CTC part when ctc_weight > 0 (score) or a scorer state is given (prune)
int m3_aed_ngram_reset(const m3_aed_joint_desc* desc, void* lm_state, size_t lm_state_bytes, const void* lm_image, size_t lm_bytes,
                    m3_stream stream) {
  return lm_reset("aed_ngram_reset", false, desc, lm_state, lm_state_bytes, lm_image, lm_bytes, nullptr, stream);
}

int m3_aed_ngram_reset_set(const m3_aed_joint_desc* desc, void* lm_state, size_t lm_state_bytes, const void* lm_image, size_t lm_bytes,
                           const int32_t* lm_on, m3_stream stream) {
  return lm_reset("aed_ngram_reset_set", true, desc, lm_state, lm_state_bytes, lm_image, lm_bytes, lm_on, stream);
}

int m3_aed_ngram_score(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                    size_t joint_state_bytes, void* scratch, size_t scratch_bytes, const void* lm_state, size_t lm_state_bytes,
                    void* lm_scratch, size_t lm_scratch_bytes, const float* logits, int ldl, const float* ctc, int ldc, int ctc_rows,
                    float ctc_weight, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha, double beta, int use_eos,
                    m3_stream stream) {
  M3_REQUIRE(ctc_weight >= 0.f && ctc_weight <= 1.f, "aed_ngram_score: ctc_weight = %g outside [0, 1]", (double)ctc_weight);
  FusedCall c = fused_call("aed_ngram_score", NGRAM, ctc_weight > 0.f, true, false, desc, search_state, search_state_bytes, stream);
  M3_REQUIRE((ctc != nullptr) == c.ctc || c.empty(), "aed_ngram_score: the CTC log-probabilities are given exactly when ctc_weight > 0 (ctc_weight = %g)",
             (double)ctc_weight);
  c.js = joint_state, c.js_bytes = joint_state_bytes, c.scr = scratch, c.scr_bytes = scratch_bytes;
  c.x = ctc, c.ldx = ldc, c.x_rows = ctc_rows, c.lam = ctc_weight;
  c.ls = lm_state, c.ls_bytes = lm_state_bytes, c.lscr = lm_scratch, c.lscr_bytes = lm_scratch_bytes;
  c.image = lm_image, c.image_bytes = lm_bytes, c.lm_on = lm_on, c.alpha = alpha, c.beta = beta, c.use_eos = use_eos;
  c.logits = logits, c.ldl = ldl;
  return fused_score(c);
}

int m3_aed_ngram_prune(const m3_aed_joint_desc* desc, void* search_state, size_t search_state_bytes, void* joint_state, size_t joint_state_bytes,
                    const void* scratch, size_t scratch_bytes, void* lm_state, size_t lm_state_bytes, const void* lm_scratch,
                    size_t lm_scratch_bytes, int32_t* done, m3_stream stream) {
  // the CTC = false form has no scorer state
  FusedCall c = fused_call("aed_ngram_prune", NGRAM, joint_state != nullptr, true, false, desc, search_state, search_state_bytes, stream);
  c.js = joint_state, c.js_bytes = joint_state_bytes, c.scr = scratch, c.scr_bytes = scratch_bytes;
  c.ls = lm_state, c.ls_bytes = lm_state_bytes, c.lscr = lm_scratch, c.lscr_bytes = lm_scratch_bytes;
  c.done = done;
  return fused_prune(c);
}

int m3_aed_ngram_result(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* lm_state,
                     size_t lm_state_bytes, float* lm, int32_t* lm_state_out, int32_t* n, float* att, m3_stream stream) {
  FusedCall c = fused_call("aed_ngram_result", NGRAM, false, true, false, desc, search_state, search_state_bytes, stream);
  c.ls = lm_state, c.ls_bytes = lm_state_bytes;
  if (int rc = check_call(c, false, false)) return rc;
  if (desc->search.B == 0) return 0;
  M3_REQUIRE(lm && lm_state_out, "aed_ngram_result: null pointer");
  hipLaunchKernelGGL(aed_lm_result_kernel, dim3((unsigned)desc->search.B), dim3(64), 0, c.stream, (const int32_t*)search_state,
                     desc->search.beam, search_layout(&desc->search).P, (const int32_t*)lm_state, lm, lm_state_out, n, att);
  M3_LAUNCH_CHECK();
  return 0;
}

// ---- m3_aed_bias_*: always the context part; the CTC and LM parts as ctc_weight and the pointers say
int m3_aed_bias_reset(const m3_aed_joint_desc* desc, const m3_aed_bias* bias, m3_stream stream) {
  if (int rc = check_desc(desc, BIAS, false)) return rc;
  if (int rc = check_bias(desc, bias, true, false, "aed_bias_reset")) return rc;
  // the image's header, read back once per search: what ctx_graph_view refuses here the kernels would run as "unbiased"
  int32_t head[CTX_HDR_WORDS];
  M3_CHECK_HIP(hipMemcpy(head, bias->image, sizeof(head), hipMemcpyDeviceToHost));
  M3_REQUIRE(head[CTX_MAGIC] == kCtxMagic && head[CTX_G] >= 0 && head[CTX_G] <= kCtxMaxGraphs &&
                 CTX_HDR_WORDS + (long long)head[CTX_G] * CTXG_WORDS <= (long long)(bias->image_bytes / 4),
             "aed_bias_reset: the image's header does not describe a context set of %zu bytes", bias->image_bytes);
  M3_REQUIRE(head[CTX_V] == desc->search.V, "aed_bias_reset: the context image was built for V = %d, the search has V = %d", head[CTX_V],
             desc->search.V);
  if (desc->search.B == 0) return 0;
  const int R = desc->search.B * desc->search.beam;
  hipLaunchKernelGGL(aed_bias_reset_kernel, dim3((unsigned)cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, R, desc->search.beam, (int32_t*)bias->state);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_bias_score(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                      size_t joint_state_bytes, void* scratch, size_t scratch_bytes, const void* lm_state, size_t lm_state_bytes,
                      void* lm_scratch, size_t lm_scratch_bytes, const float* logits, int ldl, const float* ctc, int ldc, int ctc_rows,
                      float ctc_weight, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha, double beta, int use_eos,
                      const m3_aed_bias* bias, m3_stream stream) {
  M3_REQUIRE(ctc_weight >= 0.f && ctc_weight <= 1.f, "aed_bias_score: ctc_weight = %g outside [0, 1]", (double)ctc_weight);
  FusedCall c = fused_call("aed_bias_score", BIAS, ctc_weight > 0.f, lm_image != nullptr, true, desc, search_state, search_state_bytes, stream);
  M3_REQUIRE((ctc != nullptr) == c.ctc || c.empty(), "aed_bias_score: the CTC log-probabilities are given exactly when ctc_weight > 0 (ctc_weight = %g)",
             (double)ctc_weight);
  M3_REQUIRE(((joint_state != nullptr) == c.ctc && (scratch != nullptr) == c.ctc) || c.empty(),
             "aed_bias_score: the scorer state and the joint scratch are given exactly when ctc_weight > 0 (ctc_weight = %g)", (double)ctc_weight);
  M3_REQUIRE(((lm_state != nullptr) == c.lm && (lm_scratch != nullptr) == c.lm && (lm_on != nullptr) == c.lm) || c.empty(),
             "aed_bias_score: the LM image, lm_on, the LM state and the LM scratch are NULL exactly when there is no LM");
  c.js = joint_state, c.js_bytes = joint_state_bytes, c.scr = scratch, c.scr_bytes = scratch_bytes;
  c.x = ctc, c.ldx = ldc, c.x_rows = ctc_rows, c.lam = ctc_weight;
  c.ls = lm_state, c.ls_bytes = lm_state_bytes, c.lscr = lm_scratch, c.lscr_bytes = lm_scratch_bytes;
  c.image = lm_image, c.image_bytes = lm_bytes, c.lm_on = lm_on, c.alpha = alpha, c.beta = beta, c.use_eos = use_eos;
  c.bias = bias, c.logits = logits, c.ldl = ldl;
  return fused_score(c);
}

int m3_aed_bias_prune(const m3_aed_joint_desc* desc, void* search_state, size_t search_state_bytes, void* joint_state, size_t joint_state_bytes,
                      const void* scratch, size_t scratch_bytes, void* lm_state, size_t lm_state_bytes, const void* lm_scratch,
                      size_t lm_scratch_bytes, const m3_aed_bias* bias, int32_t* done, m3_stream stream) {
  // the parts as the score call of the same search had them
  FusedCall c = fused_call("aed_bias_prune", BIAS, joint_state != nullptr, lm_state != nullptr, true, desc, search_state, search_state_bytes, stream);
  M3_REQUIRE((scratch != nullptr) == c.ctc || c.empty(), "aed_bias_prune: the scorer state and the joint scratch are given together or not at all");
  M3_REQUIRE((lm_scratch != nullptr) == c.lm || c.empty(), "aed_bias_prune: the LM state and the LM scratch are given together or not at all");
  c.js = joint_state, c.js_bytes = joint_state_bytes, c.scr = scratch, c.scr_bytes = scratch_bytes;
  c.ls = lm_state, c.ls_bytes = lm_state_bytes, c.lscr = lm_scratch, c.lscr_bytes = lm_scratch_bytes;
  c.bias = bias, c.done = done;
  return fused_prune(c);
}

int m3_aed_bias_result(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const m3_aed_bias* bias,
                       float* bonus, int32_t* ctx_state, float* att, m3_stream stream) {
  FusedCall c = fused_call("aed_bias_result", BIAS, false, false, true, desc, search_state, search_state_bytes, stream);
  c.bias = bias;
  if (int rc = check_call(c, false, false)) return rc;
  if (desc->search.B == 0) return 0;
  M3_REQUIRE(bonus && ctx_state, "aed_bias_result: null pointer");
  hipLaunchKernelGGL(aed_bias_result_kernel, dim3((unsigned)desc->search.B), dim3(64), 0, c.stream, (const int32_t*)search_state,
                     desc->search.beam, search_layout(&desc->search).P, (const int32_t*)bias->state, bonus, ctx_state, att);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
