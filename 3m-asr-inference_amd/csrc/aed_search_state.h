// The state blob of attention decoding and the pick order of its pruning step, shared by csrc/aed_search.hip and
// csrc/aed_joint.hip: the joint CTC/attention step reads and writes the SAME records and headers.
//
//   state (int32 words):  [ B headers of AS_HDR words: step, limit, done, mem_row0, mem_len ]
//                         [ R rows of 2 records (double buffer); record = score, finished, tokens[P], path[P] ],  P = max_steps + 1
#pragma once
#include <limits.h>
#include <math.h>

#include "../../include/m3asr.h"
#include "common.h"

namespace m3 {

enum { AS_STEP = 0, AS_LIMIT = 1, AS_DONE = 2, AS_MEM_ROW0 = 3, AS_MEM_LEN = 4, AS_HDR = 8 };
enum { AS_SCORE = 0, AS_FINISHED = 1, AS_TOKENS = 2 };
constexpr int AS_MAX_BEAM = 64;

struct SearchLayout {
  int P;           // token / path positions per record
  int rec_words;   // one record
  int row_words;   // both records of a row
};

static inline SearchLayout search_layout(const m3_aed_search_desc* d) {
  SearchLayout l;
  l.P = d->max_steps + 1;
  l.rec_words = AS_TOKENS + 2 * l.P;
  l.row_words = 2 * l.rec_words;
  return l;
}

static inline int check_search_desc(const m3_aed_search_desc* d) {
  M3_REQUIRE(d != nullptr, "aed_search: null descriptor");
  M3_REQUIRE(d->B >= 0 && d->B <= 65535, "aed_search: B = %d outside [0, 65535]", d->B);
  M3_REQUIRE(d->V >= 1 && d->V <= (1 << 24), "aed_search: V = %d outside [1, 2^24]", d->V);
  M3_REQUIRE(d->beam >= 1 && d->beam <= AS_MAX_BEAM && d->beam <= d->V, "aed_search: beam = %d, need 1 <= beam <= min(%d, V = %d)",
             d->beam, AS_MAX_BEAM, d->V);
  M3_REQUIRE(d->max_steps >= 1 && d->max_steps <= (1 << 16), "aed_search: max_steps = %d outside [1, 2^16]", d->max_steps);
  M3_REQUIRE(d->H >= 1 && d->D >= 16 && d->D <= (1 << 16) && d->D % d->H == 0, "aed_search: D = %d, H = %d", d->D, d->H);
  const int dk = d->D / d->H;
  M3_REQUIRE(dk % 16 == 0 && dk <= 128, "aed_search: head size %d; the attention kernel takes multiples of 16 up to 128", dk);
  M3_REQUIRE(d->layers >= 1 && d->layers <= 4096, "aed_search: layers = %d outside [1, 4096]", d->layers);
  M3_REQUIRE(d->pe_rows >= 2, "aed_search: pe_rows = %d, the positional table needs at least 2 rows", d->pe_rows);
  const size_t R = (size_t)d->B * d->beam;
  M3_REQUIRE(R * (size_t)search_layout(d).row_words + (size_t)d->B * AS_HDR <= (size_t)INT_MAX,
             "aed_search: %zu rows of %d steps overflow the int32 state offsets", R, d->max_steps);
  M3_REQUIRE((size_t)d->layers * d->max_steps * R <= (size_t)INT_MAX,
             "aed_search: %d layers x %d steps x %zu rows overflow the int32 row index of the K / V cache", d->layers, d->max_steps, R);
  M3_REQUIRE(R * (size_t)d->H <= (size_t)INT_MAX / 2, "aed_search: %zu rows x %d heads overflow the attention grid", R, d->H);
  return 0;
}

static inline size_t search_state_bytes(const m3_aed_search_desc* d) {
  const size_t R = (size_t)d->B * d->beam;
  return align_up(4 * ((size_t)d->B * AS_HDR + R * (size_t)search_layout(d).row_words), 256);
}

static inline int check_search_state(const m3_aed_search_desc* d, const void* state, size_t bytes, const char* what) {
  if (int rc = check_search_desc(d)) return rc;
  M3_REQUIRE(bytes >= search_state_bytes(d), "%s: state %zu bytes < required %zu", what, bytes, search_state_bytes(d));
  M3_REQUIRE(d->B == 0 || (state != nullptr && ((uintptr_t)state & 15) == 0), "%s: the state must be 16-byte aligned device memory", what);
  return 0;
}

__device__ __forceinline__ const int32_t* as_header(const int32_t* st, int u) { return st + (size_t)u * AS_HDR; }
__device__ __forceinline__ const int32_t* as_record(const int32_t* st, int B, int rec_words, int row, int buf) {
  return st + (size_t)B * AS_HDR + ((size_t)row * 2 + buf) * rec_words;
}
__device__ __forceinline__ int lane_bcast_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float lane_bcast_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// the larger of two (value, index) candidates: larger value, then lower index; index < 0 = none
__device__ __forceinline__ void better_of(float& v, int& i, float ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
    v = ov;
    i = oi;
  }
}
__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    better_of(v, i, ov, oi);
  }
}
// the best of n entries that comes AFTER (pv, pi) in the order (value descending, index ascending); first: no predecessor.
// Every lane returns the same pair; NaN entries are never chosen.
__device__ __forceinline__ void wave_next_best(const float* x, int n, bool first, float pv, int pi, int lane, float& bv, int& bi) {
  bv = -INFINITY;
  bi = -1;
  for (int c = lane; c < n; c += 64) {
    const float v = x[c];
    const bool after = first ? (v == v) : (v < pv || (v == pv && c > pi));
    if (after && (bi < 0 || v > bv)) {                            // c ascends within a lane: a tie keeps the lower index
      bv = v;
      bi = c;
    }
  }
  wave_best(bv, bi);
}

}  // namespace m3
