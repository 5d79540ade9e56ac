// CTC decoding through a compiled graph (TLG): Viterbi token passing with one token per graph state, on the device
// (include/m3asr.h "WFST decoding").  One work-group of 1024 threads per utterance, all frames of a call in
// one launch, all state in caller-owned memory, so a search resumes at any frame boundary.
//
//   host    wfst_validate            the image check m3asr.wfst.DecodingGraph.to() runs before it uploads
//   device  wfst_clear_kernel        reset, part 1: both dense key arrays of the selected utterances to "no token"
//           wfst_start_kernel        reset, part 2: the start token and its epsilon closure
//           wfst_advance_kernel      the frames of one call: choose, emit, cut, epsilon closure by level
//           wfst_result_kernel       best live token (with or without final weights) and its word sequence
//
// Nothing depends on thread order: every token update is a 64-bit atomic min of (ordered cost bits << 32 | arc id), the set
// of states a phase touches and the number of records it makes are properties of the data, and every decision that ends a
// frame early is taken by all threads from values that no thread changes before the next barrier.
#include <math.h>

#include <vector>

#include "../../include/m3asr.h"
#include "common.h"
#include "kernels.h"

namespace m3 {
namespace {

typedef unsigned long long u64;

constexpr int32_t kFstMagic = 0x5346334D;   // "M3FS"
constexpr int32_t kFstVersion = 1;
constexpr int kFstHdrWords = 20;
constexpr int kFstMaxStates = 1 << 26;
constexpr int kFstMaxLevels = 64;
constexpr size_t kFstMaxBytes = (size_t)1 << 30;
constexpr int kFstMaxV = 12288;             // the frame's row lives in LDS
enum { FST_MAGIC = 0, FST_VERSION, FST_V, FST_STATES, FST_ARCS, FST_START, FST_LEVELS, FST_RESERVED, FST_TABLES = 8, FST_WORDS = 16 };
enum { T_ARC_BEGIN = 0, T_EPS_BEGIN, T_ILABEL, T_OLABEL, T_DST, T_WEIGHT, T_FINAL, T_EPS_LEVEL, T_COUNT };

struct FstView {
  int V, n_states, n_arcs, start, n_levels;
  const int32_t *arc_begin, *eps_begin, *ilabel, *olabel, *dst, *eps_level;
  const float *weight, *fin;
};

__host__ __device__ inline bool fst_table(const int32_t* w, long long words, int i, long long len, const int32_t** out) {
  const long long off = w[FST_TABLES + i];
  if (off < kFstHdrWords || off + len > words) return false;
  *out = w + off;
  return true;
}

// The header's numbers inside their limits and every table inside the image.  Host and device: the kernels run it on the
// device image before they form an address from it.
__host__ __device__ inline bool fst_view(const int32_t* w, long long words, FstView* g) {
  if (words < kFstHdrWords || w[FST_MAGIC] != kFstMagic || w[FST_VERSION] != kFstVersion) return false;
  g->V = w[FST_V];
  g->n_states = w[FST_STATES];
  g->n_arcs = w[FST_ARCS];
  g->start = w[FST_START];
  g->n_levels = w[FST_LEVELS];
  if (g->V < 1 || g->n_states < 1 || g->n_states > kFstMaxStates || g->n_arcs < 0 || g->start < 0 || g->start >= g->n_states ||
      g->n_levels < 1 || g->n_levels > kFstMaxLevels)
    return false;
  const long long N = g->n_states, A = g->n_arcs;
  // (no pointer array here: indexed at run time it would live in scratch memory)
  return fst_table(w, words, T_ARC_BEGIN, N + 1, &g->arc_begin) && fst_table(w, words, T_EPS_BEGIN, N, &g->eps_begin) &&
         fst_table(w, words, T_ILABEL, A, &g->ilabel) && fst_table(w, words, T_OLABEL, A, &g->olabel) &&
         fst_table(w, words, T_DST, A, &g->dst) && fst_table(w, words, T_WEIGHT, A, (const int32_t**)&g->weight) &&
         fst_table(w, words, T_FINAL, N, (const int32_t**)&g->fin) && fst_table(w, words, T_EPS_LEVEL, N, &g->eps_level);
}

}  // namespace

// ------------------------------------------------------------------------------------------ the validator (host)
int wfst_validate(const void* image, size_t bytes, int V) {
  M3_REQUIRE(image != nullptr, "wfst_validate: null image");
  M3_REQUIRE(V >= 1, "wfst_validate: V = %d < 1", V);
  M3_REQUIRE(bytes % 4 == 0 && bytes >= (size_t)kFstHdrWords * 4 && bytes <= kFstMaxBytes,
             "wfst_validate: image of %zu bytes (a multiple of 4 in [%d, %zu])", bytes, kFstHdrWords * 4, kFstMaxBytes);
  const int32_t* w = (const int32_t*)image;
  const long long words = (long long)(bytes / 4);
  M3_REQUIRE(w[FST_MAGIC] == kFstMagic, "wfst_validate: not a graph image");
  M3_REQUIRE(w[FST_VERSION] == kFstVersion, "wfst_validate: image version %d, this library reads version %d", w[FST_VERSION], kFstVersion);
  M3_REQUIRE(w[FST_V] == V, "wfst_validate: image built for V = %d, asked for V = %d", w[FST_V], V);
  M3_REQUIRE(w[FST_WORDS] == words, "wfst_validate: image says %d words, has %lld", w[FST_WORDS], words);
  M3_REQUIRE(w[FST_STATES] <= kFstMaxStates, "wfst_validate: n_states = %d > %d", w[FST_STATES], kFstMaxStates);
  M3_REQUIRE(w[FST_LEVELS] <= kFstMaxLevels, "wfst_validate: n_levels = %d > %d", w[FST_LEVELS], kFstMaxLevels);
  FstView g;
  M3_REQUIRE(fst_view(w, words, &g),
             "wfst_validate: n_states outside [1, %d], n_arcs < 0, start outside [0, n_states), n_levels outside [1, %d] or a table "
             "outside the image", kFstMaxStates, kFstMaxLevels);
  const int N = g.n_states, A = g.n_arcs;
  M3_REQUIRE(g.arc_begin[0] == 0 && g.arc_begin[N] == A, "wfst_validate: arc_begin[0] = %d, arc_begin[n_states] = %d, n_arcs = %d",
             g.arc_begin[0], g.arc_begin[N], A);
  for (int s = 0; s < N; ++s) {
    const int lo = g.arc_begin[s], hi = g.arc_begin[s + 1], eb = g.eps_begin[s];
    M3_REQUIRE(lo >= 0 && lo <= hi && hi <= A, "wfst_validate: arc_begin[%d..] = %d, %d is not monotone in [0, %d]", s, lo, hi, A);
    M3_REQUIRE(eb >= lo && eb <= hi, "wfst_validate: eps_begin[%d] = %d outside [%d, %d]", s, eb, lo, hi);
  }
  bool any_final = false;
  for (int s = 0; s < N; ++s) {
    const float f = g.fin[s];
    M3_REQUIRE(!std::isnan(f) && !(std::isinf(f) && f < 0.f), "wfst_validate: final[%d] is NaN or -inf", s);
    M3_REQUIRE(!(f == 0.f && std::signbit(f)), "wfst_validate: final[%d] is -0.0", s);
    any_final = any_final || std::isfinite(f);
  }
  M3_REQUIRE(any_final, "wfst_validate: no final state");
  std::vector<int32_t> indeg((size_t)N, 0);
  for (int s = 0; s < N; ++s) {
    const int lo = g.arc_begin[s], hi = g.arc_begin[s + 1], eb = g.eps_begin[s];
    for (int a = lo; a < hi; ++a) {
      const int il = g.ilabel[a], d = g.dst[a];
      M3_REQUIRE(il >= 0 && il <= V, "wfst_validate: arc %d: ilabel = %d outside [0, %d]", a, il, V);
      M3_REQUIRE((a < eb) == (il != 0), "wfst_validate: arc %d of state %d: ilabel = %d on the wrong side of eps_begin = %d", a, s, il, eb);
      M3_REQUIRE(g.olabel[a] >= 0, "wfst_validate: arc %d: olabel = %d < 0", a, g.olabel[a]);
      M3_REQUIRE(d >= 0 && d < N, "wfst_validate: arc %d: dst = %d outside [0, %d)", a, d, N);
      M3_REQUIRE(std::isfinite(g.weight[a]), "wfst_validate: arc %d: weight is not finite", a);
      M3_REQUIRE(!(g.weight[a] == 0.f && std::signbit(g.weight[a])), "wfst_validate: arc %d: weight is -0.0", a);
      if (a > lo && a != eb)
        M3_REQUIRE(g.ilabel[a - 1] < il || (g.ilabel[a - 1] == il && g.dst[a - 1] <= d),
                   "wfst_validate: arcs %d, %d of state %d are not sorted by (ilabel, dst)", a - 1, a, s);
      if (il == 0) ++indeg[d];
    }
  }
  // eps_level = longest path of epsilon-input arcs ending in the state: Kahn's order over the epsilon-input subgraph
  std::vector<int32_t> level((size_t)N, 0), queue;
  queue.reserve((size_t)N);
  for (int s = 0; s < N; ++s)
    if (indeg[s] == 0) queue.push_back(s);
  for (size_t q = 0; q < queue.size(); ++q) {
    const int s = queue[q];
    for (int a = g.eps_begin[s]; a < g.arc_begin[s + 1]; ++a) {
      const int d = g.dst[a];
      if (level[d] < level[s] + 1) level[d] = level[s] + 1;
      if (--indeg[d] == 0) queue.push_back(d);
    }
  }
  if (queue.size() < (size_t)N) {
    // every state left has a predecessor that is left: walk predecessors for as many steps as states are left
    std::vector<int32_t> pred((size_t)N, -1);
    int at = -1;
    for (int s = 0; s < N; ++s) {
      if (indeg[s] <= 0) continue;
      at = s;
      for (int a = g.eps_begin[s]; a < g.arc_begin[s + 1]; ++a)
        if (indeg[g.dst[a]] > 0) pred[g.dst[a]] = s;
    }
    for (size_t i = queue.size(); i < (size_t)N && at >= 0 && pred[at] >= 0; ++i) at = pred[at];
    M3_REQUIRE(false, "wfst_validate: the epsilon-input arcs form a cycle through state %d", at);
  }
  int top = 0;
  for (int s = 0; s < N; ++s) {
    M3_REQUIRE(g.eps_level[s] == level[s], "wfst_validate: eps_level[%d] = %d, the longest epsilon path ending there has %d arcs", s,
               g.eps_level[s], level[s]);
    if (level[s] > top) top = level[s];
  }
  M3_REQUIRE(top + 1 <= kFstMaxLevels, "wfst_validate: n_levels = %d > %d", top + 1, kFstMaxLevels);
  M3_REQUIRE(g.n_levels == top + 1, "wfst_validate: n_levels = %d, the deepest eps_level is %d", g.n_levels, top);
  return 0;
}

// ------------------------------------------------------------------------------------------ state layout
namespace {

constexpr u64 kEmpty = ~0ull;
constexpr unsigned kNoArc = 0xFFFFFFFFu;
constexpr int kThreads = 1024;
constexpr int kBigDegree = 32;              // a token with more emitting arcs is expanded by a whole wave
constexpr int kBigCap = 2048;
enum { H_PARITY = 0, H_NTOUCH, H_CUTOFF, H_T, H_NREC, H_STATUS, H_WORDS = 16 };

struct Layout {   // byte offsets inside one utterance's state
  size_t key, hist, touched, level, rec, total;
};
__host__ __device__ inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
__host__ __device__ inline Layout wfst_layout(int n_states, int n_levels, int token_cap, int record_cap) {
  Layout l;
  size_t off = H_WORDS * 4;
  l.key = off;      off += (size_t)2 * n_states * 8;
  l.hist = off;     off += up16((size_t)2 * n_states * 4);
  l.touched = off;  off += up16((size_t)2 * token_cap * 4);
  l.level = off;    off += up16((size_t)n_levels * token_cap * 4);
  l.rec = off;      off += up16((size_t)3 * record_cap * 4);
  l.total = (off + 255) & ~(size_t)255;
  return l;
}

struct Args {
  char* state;
  Layout lay;
  const int32_t* image;
  long long words;
  const int32_t* slots;     // reset: the utterances to restart (NULL = block index)
  const float* logp;
  const int32_t* n_frames;
  int ld, T_chunk;
  int N, n_levels, V, token_cap, record_cap, max_frames, max_active;
  float beam, ascale;
};

__device__ __forceinline__ unsigned f2o(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float o2f(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
__device__ __forceinline__ bool finite_f(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ u64 load_key(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct Shared {
  u64 sel;                       // (a): the max_active-th smallest (cost, state) key; a token above it is not expanded
  u64 prefix, mask;              // the radix select's state
  unsigned best, best_e;         // ordered bits of the smallest live cost / the smallest emitted cost
  unsigned bins[256];
  int lvl_cnt[kFstMaxLevels];
  int over[kFstMaxLevels + 1];   // over[p]: phase p (0 = emit, L + 1 = level L) touched more than token_cap states
  int big[kBigCap];
  int n_next, n_rec, n_exp, n_big, k_rem;
};

struct Utt {      // one utterance's arrays; cur / next by parity (computed, not indexed: a pointer array would live in scratch)
  int32_t* hdr;
  u64* key0;
  int32_t *hist0, *touched0;
  int32_t* level;
  int32_t *rec_prev, *rec_olabel, *rec_frame;
  int N, cap;
  __device__ __forceinline__ u64* key(int p) const { return key0 + (size_t)p * N; }
  __device__ __forceinline__ int32_t* hist(int p) const { return hist0 + (size_t)p * N; }
  __device__ __forceinline__ int32_t* touched(int p) const { return touched0 + (size_t)p * cap; }
};
__device__ __forceinline__ Utt utt_view(char* base, const Layout& l, int N, int token_cap, int record_cap) {
  Utt u;
  u.hdr = (int32_t*)base;
  u.key0 = (u64*)(base + l.key);
  u.hist0 = (int32_t*)(base + l.hist);
  u.touched0 = (int32_t*)(base + l.touched);
  u.N = N;
  u.cap = token_cap;
  u.level = (int32_t*)(base + l.level);
  u.rec_prev = (int32_t*)(base + l.rec);
  u.rec_olabel = u.rec_prev + record_cap;
  u.rec_frame = u.rec_olabel + record_cap;
  return u;
}

// min into next[dst]; the thread that finds the state empty lists it (touched list, its level's worklist)
__device__ __forceinline__ void push(const Args& a, const FstView& g, Shared& sh, u64* nkey, int32_t* ntouched, int32_t* level,
                                     int phase, int dst, float cand, unsigned arc) {
  const u64 k = ((u64)f2o(cand) << 32) | arc;
  const u64 old = atomicMin(&nkey[dst], k);
  if (old != kEmpty) return;
  const int i = atomicAdd(&sh.n_next, 1);
  if (i < a.token_cap) ntouched[i] = dst; else sh.over[phase] = 1;
  const int L = g.eps_level[dst];
  if ((unsigned)L < (unsigned)a.n_levels) {
    const int j = atomicAdd(&sh.lvl_cnt[L], 1);
    if (j < a.token_cap) level[(size_t)L * a.token_cap + j] = dst;
  }
}

// the state an arc leaves: the last s with arc_begin[s] <= arc
__device__ __forceinline__ int arc_source(const FstView& g, int arc) {
  int lo = 0, hi = g.n_states - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g.arc_begin[mid + 1] > arc) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Step (d).  Entered with every push of the phase before it issued but not yet behind a barrier.  Returns the status bits it
// raises (the same value in every thread); leaves behind a barrier.
__device__ int closure(const Args& a, const FstView& g, Shared& sh, const Utt& u, int nx, int t, float cutoff) {
  u64* nkey = u.key(nx);
  int32_t *nhist = u.hist(nx), *chist = u.hist(nx ^ 1), *ntouched = u.touched(nx);
  const int tid = threadIdx.x;
  int status = 0;
  for (int L = 0; L < a.n_levels; ++L) {
    __syncthreads();
    if (sh.over[L]) { status = M3_WFST_TOKEN_CAP; break; }      // written in phase L - 1 only: every thread reads the same
    const int cnt = min(sh.lvl_cnt[L], a.token_cap);
    const int32_t* list = u.level + (size_t)L * a.token_cap;
    for (int i = tid; i < cnt; i += kThreads) {
      const int s = list[i];
      const u64 k = load_key(&nkey[s]);
      const float c = o2f((unsigned)(k >> 32));
      if (!(c <= cutoff)) continue;                              // cut in (c): not a live token
      const unsigned arc = (unsigned)k;
      int h = -1;
      if (arc != kNoArc && arc < (unsigned)g.n_arcs) {
        const int src = arc_source(g, (int)arc);
        h = g.ilabel[arc] != 0 ? chist[src] : nhist[src];
        const int ol = g.olabel[arc];
        if (ol != 0) {
          const int r = atomicAdd(&sh.n_rec, 1);
          if (r < a.record_cap) {
            u.rec_prev[r] = h;
            u.rec_olabel[r] = ol;
            u.rec_frame[r] = t;
            h = r;
          } else {
            h = -1;
          }
        }
      }
      nhist[s] = h;
      int lo = g.eps_begin[s], hi = g.arc_begin[s + 1];
      if (lo < 0 || hi > g.n_arcs) continue;
      for (int e = lo; e < hi; ++e) {
        const float cand = __fadd_rn(c, g.weight[e]);
        const int d = g.dst[e];
        if (finite_f(cand) && cand <= cutoff && (unsigned)d < (unsigned)g.n_states)
          push(a, g, sh, nkey, ntouched, u.level, L + 1, d, cand, (unsigned)e);
      }
    }
  }
  __syncthreads();
  if (!status && sh.over[a.n_levels]) status = M3_WFST_TOKEN_CAP;
  if (sh.n_rec > a.record_cap) status |= M3_WFST_RECORD_CAP;
  return status;
}

__device__ __forceinline__ void shared_frame_init(Shared& sh, int n_rec_keep) {
  const int tid = threadIdx.x;
  if (tid < kFstMaxLevels) sh.lvl_cnt[tid] = 0;
  if (tid <= kFstMaxLevels) sh.over[tid] = 0;
  if (tid == 0) {
    sh.sel = kEmpty;
    sh.best = sh.best_e = 0xFFFFFFFFu;
    sh.n_next = sh.n_exp = sh.n_big = 0;
    sh.n_rec = n_rec_keep;
  }
}

// ------------------------------------------------------------------------------------------ reset
__global__ void wfst_clear_kernel(Args a) {
  const int b = a.slots ? a.slots[blockIdx.y] : (int)blockIdx.y;
  u64* key = (u64*)(a.state + (size_t)b * a.lay.total + a.lay.key);
  const size_t n = (size_t)2 * a.N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) key[i] = kEmpty;
}

__global__ __launch_bounds__(kThreads) void wfst_start_kernel(Args a) {
  __shared__ Shared sh;
  const int b = a.slots ? a.slots[blockIdx.x] : (int)blockIdx.x;
  const Utt u = utt_view(a.state + (size_t)b * a.lay.total, a.lay, a.N, a.token_cap, a.record_cap);
  FstView g;
  const bool ok = fst_view(a.image, a.words, &g) && g.V == a.V && g.n_states == a.N && g.n_levels <= a.n_levels;
  shared_frame_init(sh, 0);
  __syncthreads();
  int status = M3_WFST_BAD_GRAPH;
  const float cutoff = __fadd_rn(0.0f, a.beam);
  if (ok) {
    if (threadIdx.x == 0) push(a, g, sh, u.key(0), u.touched(0), u.level, 0, g.start, 0.0f, kNoArc);
    status = closure(a, g, sh, u, 0, 0, cutoff);
  }
  if (threadIdx.x == 0) {
    u.hdr[H_PARITY] = 0;
    u.hdr[H_NTOUCH] = ok ? min(sh.n_next, a.token_cap) : 0;
    u.hdr[H_CUTOFF] = __float_as_int(cutoff);
    u.hdr[H_T] = 0;
    u.hdr[H_NREC] = ok ? min(sh.n_rec, a.record_cap) : 0;
    u.hdr[H_STATUS] = status;
  }
}

// ------------------------------------------------------------------------------------------ advance
__global__ __launch_bounds__(kThreads) void wfst_advance_kernel(Args a) {
  __shared__ Shared sh;
  extern __shared__ float row[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Utt u = utt_view(a.state + (size_t)b * a.lay.total, a.lay, a.N, a.token_cap, a.record_cap);
  int n = a.n_frames[b];
  n = n < 0 ? 0 : (n > a.T_chunk ? a.T_chunk : n);
  int status = u.hdr[H_STATUS];
  if (n == 0 || status != 0) return;
  FstView g;
  if (!(fst_view(a.image, a.words, &g) && g.V == a.V && g.n_states == a.N && g.n_levels <= a.n_levels)) {
    if (tid == 0) u.hdr[H_STATUS] = M3_WFST_BAD_GRAPH;
    return;
  }
  int cur = u.hdr[H_PARITY] & 1, n_cur = min(max(u.hdr[H_NTOUCH], 0), a.token_cap), t = u.hdr[H_T];
  float cutoff_cur = __int_as_float(u.hdr[H_CUTOFF]);
  const int n_rec0 = min(max(u.hdr[H_NREC], 0), a.record_cap);
  const float* lp = a.logp + (size_t)b * a.T_chunk * a.ld;
  const float nscale = -a.ascale;
  __syncthreads();                                               // the header is read before thread 0 may rewrite it
  if (tid == 0) sh.n_rec = n_rec0;

  for (int f = 0; f < n; ++f, lp += a.ld) {
    if (t >= a.max_frames) { status = M3_WFST_MAX_FRAMES; break; }
    const u64* ckey = u.key(cur);
    const int32_t* ctouched = u.touched(cur);
    u64* nkey = u.key(cur ^ 1);
    int32_t* ntouched = u.touched(cur ^ 1);
    __syncthreads();                                             // the frame before is done with row and sh
    for (int v = tid; v < a.V; v += kThreads) row[v] = lp[v];
    shared_frame_init(sh, sh.n_rec);
    __syncthreads();
    // ---- (a) the expandable tokens
    {
      unsigned m = 0xFFFFFFFFu;
      for (int i = tid; i < n_cur; i += kThreads) {
        const unsigned o = (unsigned)(load_key(&ckey[ctouched[i]]) >> 32);
        if (o2f(o) <= cutoff_cur && o < m) m = o;
      }
      if (m != 0xFFFFFFFFu) atomicMin(&sh.best, m);
    }
    __syncthreads();
    const float thr = __fadd_rn(o2f(sh.best), a.beam);          // (no live token: best is NaN, nothing is expandable)
    {
      int c = 0;
      for (int i = tid; i < n_cur; i += kThreads) {
        const float x = o2f((unsigned)(load_key(&ckey[ctouched[i]]) >> 32));
        c += (x <= cutoff_cur && x <= thr) ? 1 : 0;
      }
      if (c) atomicAdd(&sh.n_exp, c);
    }
    __syncthreads();
    if (sh.n_exp > a.max_active) {                               // exact: radix select of the max_active-th (cost, state) key
      if (tid == 0) { sh.prefix = 0; sh.mask = 0; sh.k_rem = a.max_active; }
      for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) sh.bins[tid] = 0;
        __syncthreads();
        const u64 prefix = sh.prefix, mask = sh.mask;
        for (int i = tid; i < n_cur; i += kThreads) {
          const int s = ctouched[i];
          const unsigned o = (unsigned)(load_key(&ckey[s]) >> 32);
          const float x = o2f(o);
          const u64 sk = ((u64)o << 32) | (unsigned)s;
          if (x <= cutoff_cur && x <= thr && (sk & mask) == prefix) atomicAdd(&sh.bins[(unsigned)(sk >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          int k = sh.k_rem, d = 0;
          for (; d < 255; ++d) {
            const int c = (int)sh.bins[d];
            if (c >= k) break;
            k -= c;
          }
          sh.k_rem = k;
          sh.prefix = prefix | ((u64)d << shift);
          sh.mask = mask | (0xFFull << shift);
        }
        __syncthreads();
      }
      if (tid == 0) sh.sel = sh.prefix;
      __syncthreads();
    }
    const u64 sel = sh.sel;
    // ---- (b) emit
    unsigned my_best = 0xFFFFFFFFu;
    for (int i = tid; i < n_cur; i += kThreads) {
      const int s = ctouched[i];
      const unsigned o = (unsigned)(load_key(&ckey[s]) >> 32);
      const float c = o2f(o);
      if (!(c <= cutoff_cur && c <= thr && (((u64)o << 32) | (unsigned)s) <= sel)) continue;
      const int lo = g.arc_begin[s], hi = g.eps_begin[s];
      if (lo < 0 || hi > g.n_arcs) continue;
      if (hi - lo > kBigDegree) {
        const int j = atomicAdd(&sh.n_big, 1);
        if (j < kBigCap) { sh.big[j] = s; continue; }
      }
      for (int e = lo; e < hi; ++e) {
        const int il = g.ilabel[e], d = g.dst[e];
        if ((unsigned)(il - 1) >= (unsigned)a.V || (unsigned)d >= (unsigned)g.n_states) continue;
        const float cand = __fadd_rn(__fadd_rn(c, g.weight[e]), __fmul_rn(nscale, row[il - 1]));
        if (!finite_f(cand)) continue;
        push(a, g, sh, nkey, ntouched, u.level, 0, d, cand, (unsigned)e);
        my_best = min(my_best, f2o(cand));
      }
    }
    __syncthreads();
    {
      const int n_big = min(sh.n_big, kBigCap);
      for (int j = tid >> 6; j < n_big; j += kThreads >> 6) {
        const int s = sh.big[j];
        const float c = o2f((unsigned)(load_key(&ckey[s]) >> 32));
        const int lo = g.arc_begin[s], hi = g.eps_begin[s];
        for (int e = lo + (tid & 63); e < hi; e += 64) {
          const int il = g.ilabel[e], d = g.dst[e];
          if ((unsigned)(il - 1) >= (unsigned)a.V || (unsigned)d >= (unsigned)g.n_states) continue;
          const float cand = __fadd_rn(__fadd_rn(c, g.weight[e]), __fmul_rn(nscale, row[il - 1]));
          if (!finite_f(cand)) continue;
          push(a, g, sh, nkey, ntouched, u.level, 0, d, cand, (unsigned)e);
          my_best = min(my_best, f2o(cand));
        }
      }
    }
    if (my_best != 0xFFFFFFFFu) atomicMin(&sh.best_e, my_best);
    __syncthreads();
    // ---- (c) cut
    const unsigned best_e = sh.best_e;
    if (best_e == 0xFFFFFFFFu) { status = M3_WFST_DEAD; break; }
    const float cutoff = __fadd_rn(o2f(best_e), a.beam);
    // ---- (d) epsilon closure by level
    status = closure(a, g, sh, u, cur ^ 1, t, cutoff);
    if (status) break;
    for (int i = tid; i < n_cur; i += kThreads) u.key(cur)[ctouched[i]] = kEmpty;
    n_cur = min(sh.n_next, a.token_cap);
    cutoff_cur = cutoff;
    cur ^= 1;
    ++t;
  }
  __syncthreads();
  if (tid == 0) {
    u.hdr[H_PARITY] = cur;
    u.hdr[H_NTOUCH] = n_cur;
    u.hdr[H_CUTOFF] = __float_as_int(cutoff_cur);
    u.hdr[H_T] = t;
    u.hdr[H_NREC] = min(sh.n_rec, a.record_cap);
    u.hdr[H_STATUS] = status;
  }
}

// ------------------------------------------------------------------------------------------ result
struct ResultArgs {
  int final, max_words;
  int32_t *words, *frames, *n_words, *flags, *status;
  float* cost;
};

__global__ __launch_bounds__(256) void wfst_result_kernel(Args a, ResultArgs r) {
  __shared__ u64 best_final, best_any;
  const int b = blockIdx.x, tid = threadIdx.x;
  const Utt u = utt_view(a.state + (size_t)b * a.lay.total, a.lay, a.N, a.token_cap, a.record_cap);
  const int status = u.hdr[H_STATUS];
  FstView g;
  const bool ok = fst_view(a.image, a.words, &g) && g.V == a.V && g.n_states == a.N && g.n_levels <= a.n_levels;
  if (tid == 0) { best_final = kEmpty; best_any = kEmpty; }
  __syncthreads();
  const int cur = u.hdr[H_PARITY] & 1, n_cur = min(max(u.hdr[H_NTOUCH], 0), a.token_cap);
  const float cutoff = __int_as_float(u.hdr[H_CUTOFF]);
  const bool run = ok && status == 0;
  if (run) {
    for (int i = tid; i < n_cur; i += blockDim.x) {
      const int s = u.touched(cur)[i];
      if ((unsigned)s >= (unsigned)a.N) continue;
      const float c = o2f((unsigned)(u.key(cur)[s] >> 32));
      if (!(c <= cutoff)) continue;
      atomicMin(&best_any, ((u64)f2o(c) << 32) | (unsigned)s);
      if (r.final) {
        const float tot = __fadd_rn(c, g.fin[s]);
        if (finite_f(tot)) atomicMin(&best_final, ((u64)f2o(tot) << 32) | (unsigned)s);
      }
    }
  }
  __syncthreads();
  if (tid != 0) return;
  int32_t* words = r.words + (size_t)b * r.max_words;
  int32_t* frames = r.frames + (size_t)b * r.max_words;
  int n = 0, reached = 0, st_out = ok ? status : (status | M3_WFST_BAD_GRAPH);
  float cost = __int_as_float(0x7F800000);
  if (st_out & ~M3_WFST_DEAD) {
    n = -1;
  } else if (run) {
    reached = r.final && best_final != kEmpty;
    const u64 k = reached ? best_final : best_any;
    if (k != kEmpty) {
      cost = o2f((unsigned)(k >> 32));
      const int n_rec = min(max(u.hdr[H_NREC], 0), a.record_cap);
      int len = 0;
      for (int h = u.hist(cur)[(unsigned)k]; h >= 0 && h < n_rec && len <= n_rec; h = u.rec_prev[h]) ++len;
      if (len > r.max_words) {
        n = -1;
        st_out |= M3_WFST_WORD_CAP;
      } else {
        n = len;
        int at = len;
        for (int h = u.hist(cur)[(unsigned)k]; h >= 0 && h < n_rec && at > 0; h = u.rec_prev[h]) {
          --at;
          words[at] = u.rec_olabel[h];
          frames[at] = u.rec_frame[h];
        }
      }
    }
  }
  for (int i = n < 0 ? 0 : n; i < r.max_words; ++i) { words[i] = -1; frames[i] = -1; }
  r.n_words[b] = n;
  r.cost[b] = cost;
  r.flags[b] = reached;
  r.status[b] = st_out;
}

int check_desc(const m3_wfst_search_desc* d, const char* who) {
  M3_REQUIRE(d != nullptr, "%s: null descriptor", who);
  M3_REQUIRE(d->B >= 0 && d->B <= 32768, "%s: B = %d outside [0, 32768]", who, d->B);
  M3_REQUIRE(d->max_frames >= 1, "%s: max_frames = %d < 1", who, d->max_frames);
  M3_REQUIRE(d->n_states >= 1 && d->n_states <= kFstMaxStates, "%s: n_states = %d outside [1, %d]", who, d->n_states, kFstMaxStates);
  M3_REQUIRE(d->n_levels >= 1 && d->n_levels <= kFstMaxLevels, "%s: n_levels = %d outside [1, %d]", who, d->n_levels, kFstMaxLevels);
  M3_REQUIRE(d->V >= 1 && d->V <= kFstMaxV, "%s: V = %d outside [1, %d]", who, d->V, kFstMaxV);
  M3_REQUIRE(d->token_cap >= 1 && d->token_cap <= kFstMaxStates, "%s: token_cap = %d outside [1, %d]", who, d->token_cap, kFstMaxStates);
  M3_REQUIRE(d->record_cap >= 1 && d->record_cap <= (1 << 28), "%s: record_cap = %d outside [1, 2^28]", who, d->record_cap);
  M3_REQUIRE(d->max_active >= 1, "%s: max_active = %d < 1", who, d->max_active);
  M3_REQUIRE(d->beam > 0.f, "%s: beam = %g is not above 0", who, (double)d->beam);
  M3_REQUIRE(std::isfinite(d->acoustic_scale), "%s: acoustic_scale is not finite", who);
  return 0;
}

int fill_args(const m3_wfst_search_desc* d, void* state, size_t bytes, const void* image, size_t image_bytes, const char* who, Args* a) {
  if (int rc = check_desc(d, who)) return rc;
  const Layout lay = wfst_layout(d->n_states, d->n_levels, d->token_cap, d->record_cap);
  M3_REQUIRE(state != nullptr && ((uintptr_t)state & 15) == 0, "%s: state is null or not 16-byte aligned", who);
  M3_REQUIRE(bytes >= lay.total * (size_t)d->B, "%s: state of %zu bytes < %zu", who, bytes, lay.total * (size_t)d->B);
  M3_REQUIRE(image != nullptr && ((uintptr_t)image & 3) == 0 && image_bytes % 4 == 0 && image_bytes >= (size_t)kFstHdrWords * 4 &&
                 image_bytes <= kFstMaxBytes,
             "%s: graph image is null, misaligned or of %zu bytes (a multiple of 4 in [%d, %zu])", who, image_bytes, kFstHdrWords * 4,
             kFstMaxBytes);
  *a = Args{};
  a->state = (char*)state;
  a->lay = lay;
  a->image = (const int32_t*)image;
  a->words = (long long)(image_bytes / 4);
  a->N = d->n_states;
  a->n_levels = d->n_levels;
  a->V = d->V;
  a->token_cap = d->token_cap;
  a->record_cap = d->record_cap;
  a->max_frames = d->max_frames;
  a->max_active = d->max_active;
  a->beam = d->beam;
  a->ascale = d->acoustic_scale;
  return 0;
}

}  // namespace

size_t wfst_search_state_size(const m3_wfst_search_desc* d) {
  if (check_desc(d, "wfst_search_state_size")) return 0;
  return wfst_layout(d->n_states, d->n_levels, d->token_cap, d->record_cap).total * (size_t)d->B;
}

int launch_wfst_search_reset(const m3_wfst_search_desc* d, void* state, size_t bytes, const void* image, size_t image_bytes,
                             const int32_t* slots, int n, hipStream_t stream) {
  Args a;
  if (int rc = fill_args(d, state, bytes, image, image_bytes, "wfst_search_reset", &a)) return rc;
  M3_REQUIRE(n >= 0 && n <= d->B, "wfst_search_reset: %d slots for B = %d", n, d->B);
  const int count = slots ? n : d->B;
  if (count == 0) return 0;
  a.slots = slots;                                               // (a slot outside [0, B) is the caller's error, as in m3_ctc_beam_reset_slots)
  const unsigned gx = grid1d((size_t)2 * a.N, 1024);
  hipLaunchKernelGGL(wfst_clear_kernel, dim3(gx, count), dim3(256), 0, stream, a);
  M3_LAUNCH_CHECK();
  hipLaunchKernelGGL(wfst_start_kernel, dim3(count), dim3(kThreads), 0, stream, a);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_wfst_search_advance(const m3_wfst_search_desc* d, void* state, size_t bytes, const void* image, size_t image_bytes,
                               const float* logp, int ld, int T_chunk, const int32_t* n_frames, hipStream_t stream) {
  Args a;
  if (int rc = fill_args(d, state, bytes, image, image_bytes, "wfst_search_advance", &a)) return rc;
  M3_REQUIRE(T_chunk >= 0 && ld >= d->V, "wfst_search_advance: T_chunk = %d < 0 or ld = %d < V = %d", T_chunk, ld, d->V);
  M3_REQUIRE(n_frames != nullptr && (logp != nullptr || T_chunk == 0), "wfst_search_advance: null pointer");
  if (d->B == 0 || T_chunk == 0) return 0;
  a.logp = logp;
  a.ld = ld;
  a.T_chunk = T_chunk;
  a.n_frames = n_frames;
  hipLaunchKernelGGL(wfst_advance_kernel, dim3(d->B), dim3(kThreads), (size_t)d->V * 4, stream, a);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_wfst_search_result(const m3_wfst_search_desc* d, const void* state, size_t bytes, const void* image, size_t image_bytes,
                              int final, int max_words, int32_t* words, int32_t* frames, int32_t* n_words, float* cost,
                              int32_t* flags, int32_t* status, hipStream_t stream) {
  Args a;
  if (int rc = fill_args(d, const_cast<void*>(state), bytes, image, image_bytes, "wfst_search_result", &a)) return rc;
  M3_REQUIRE(max_words >= 1, "wfst_search_result: max_words = %d < 1", max_words);
  M3_REQUIRE(words && frames && n_words && cost && flags && status, "wfst_search_result: null pointer");
  if (d->B == 0) return 0;
  ResultArgs r{final != 0, max_words, words, frames, n_words, flags, status, cost};
  hipLaunchKernelGGL(wfst_result_kernel, dim3(d->B), dim3(256), 0, stream, a, r);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
