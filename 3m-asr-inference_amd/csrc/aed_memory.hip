// Streaming two-pass decoding: the per-slot encoder memory the attention decoder attends over when a live
// stream's utterance ends.  One state blob per streaming decoder, caller-owned, laid out slot by slot:
//
//   slot b at byte b * stride:  [ AM_HEADER bytes: int32 len, int32 status, spare ][ max_frames rows of D fp32 ]
//
// The rows are copies of the chunk binding's residual stream ("x", before after_norm); nothing is computed here.  All loads
// and stores of rows are 16 bytes per lane, consecutive lanes on consecutive 16 bytes of one row.  No atomics: a slot's words
// have one writer per launch (lane 0 of the slot's own work-group, behind a barrier that every reader of the words passes
// first), and the kernels of one state run on one stream.
#include <limits.h>

#include "../../include/m3asr.h"
#include "common.h"

namespace m3 {
namespace {

enum { AM_LEN = 0, AM_STATUS = 1 };
constexpr size_t AM_HEADER = 256;   // bytes in front of a slot's rows: the rows stay 16-byte (and 256-byte) aligned
constexpr int AM_GATHER_ROWS = 16;  // rows one work-group of the gather moves

size_t am_stride(const m3_aed_memory_desc* d) { return align_up(AM_HEADER + (size_t)d->max_frames * d->D * 4, 256); }

int check_memory_desc(const m3_aed_memory_desc* d) {
  M3_REQUIRE(d != nullptr, "aed_memory: null descriptor");
  M3_REQUIRE(d->B >= 0 && d->B <= (1 << 24), "aed_memory: B = %d outside [0, 2^24]", d->B);
  M3_REQUIRE(d->max_frames >= 0 && d->max_frames <= (1 << 24), "aed_memory: max_frames = %d outside [0, 2^24]", d->max_frames);
  M3_REQUIRE(d->D >= 4 && d->D <= (1 << 16) && (d->D & 3) == 0, "aed_memory: D = %d, need a multiple of 4 in [4, 2^16]", d->D);
  return 0;
}

int check_memory_state(const m3_aed_memory_desc* d, const void* state, size_t bytes, const char* what) {
  if (int rc = check_memory_desc(d)) return rc;
  const size_t need = (size_t)d->B * am_stride(d);
  M3_REQUIRE(bytes >= need, "%s: state %zu bytes < required %zu", what, bytes, need);
  M3_REQUIRE(d->B == 0 || (state != nullptr && ((uintptr_t)state & 15) == 0), "%s: the state must be 16-byte aligned device memory", what);
  return 0;
}

__device__ __forceinline__ const int32_t* am_words(const char* state, size_t stride, int b) {
  return reinterpret_cast<const int32_t*>(state + (size_t)b * stride);
}
__device__ __forceinline__ const float* am_rows(const char* state, size_t stride, int b) {
  return reinterpret_cast<const float*>(state + (size_t)b * stride + AM_HEADER);
}
// rows of slot b a reader may touch: 0 for a failed slot, never more than the state holds
__device__ __forceinline__ int am_valid_rows(const char* state, size_t stride, int b, int max_frames) {
  const int32_t* st = am_words(state, stride, b);
  return st[AM_STATUS] != 0 ? 0 : min(max(st[AM_LEN], 0), max_frames);
}

// only the words: no kernel reads a row the slot's current stream has not written
__global__ __launch_bounds__(256) void aed_memory_reset_kernel(char* state, size_t stride, int B, const int32_t* __restrict__ slots,
                                                               int n) {
  int b = blockIdx.x * 256 + threadIdx.x;
  if (slots != nullptr) {                         // a device list of n streams (entries outside [0, B) are skipped)
    if (b >= n) return;
    b = slots[b];
    if (b < 0) return;
  }
  if (b >= B) return;
  int32_t* st = reinterpret_cast<int32_t*>(state + (size_t)b * stride);
  st[AM_LEN] = 0;
  st[AM_STATUS] = 0;
}

// one work-group per slot: every thread reads the slot's words ONCE, the group copies the chunk's rows behind the slot's
// length, passes the barrier, and only then one thread moves the length (or marks the slot) -- the read that places the rows
// cannot see the write that moves them
__global__ __launch_bounds__(256) void aed_memory_append_kernel(char* state, size_t stride, int max_frames, int D,
                                                                const float* __restrict__ x, int ldx, int T_chunk,
                                                                const int32_t* __restrict__ n_frames) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nf = min(max(n_frames[b], 0), T_chunk);
  if (nf == 0) return;                            // idle: words and rows stay byte for byte
  int32_t* st = reinterpret_cast<int32_t*>(state + (size_t)b * stride);
  const int len = st[AM_LEN], status = st[AM_STATUS];
  const bool fail = status != 0 || len < 0 || len > max_frames || nf > max_frames - len;
  if (!fail) {
    float* rows = reinterpret_cast<float*>(state + (size_t)b * stride + AM_HEADER) + (size_t)len * D;
    const float* src = x + (size_t)b * T_chunk * ldx;
    const int c4 = D >> 2, total = nf * c4;       // at most 2^14 frames of 2^14 quads: checked by the launcher
    for (int idx = tid; idx < total; idx += 256) {
      const int r = idx / c4, c = idx - r * c4;
      stg4(rows + (size_t)r * D + 4 * c, ldg4(src + (size_t)r * ldx + 4 * c));
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (fail) st[AM_STATUS] = status ? status : 1;      // consumes nothing, stays failed until the slot is reset
    else st[AM_LEN] = len + nf;
  }
}

__global__ __launch_bounds__(256) void aed_memory_lengths_kernel(const char* __restrict__ state, size_t stride, int B,
                                                                 int max_frames, int32_t* __restrict__ len) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int32_t* st = am_words(state, stride, b);
  len[b] = st[AM_STATUS] != 0 ? -1 : min(max(st[AM_LEN], 0), max_frames);
}

// grid (listed slot j, row tile): the group sums the lengths of the slots listed before its own (n is a handful), then moves
// its AM_GATHER_ROWS rows; tile 0 writes the prefix sums
__global__ __launch_bounds__(256) void aed_memory_gather_kernel(const char* __restrict__ state, size_t stride, int B, int max_frames,
                                                                int D, const int32_t* __restrict__ slots, float* __restrict__ out,
                                                                int ldo, int out_rows, int32_t* __restrict__ out_row0) {
  const int j = blockIdx.x, tid = threadIdx.x;
  int start = 0;
  for (int i = 0; i < j; ++i) {
    const int s = slots[i];
    if (s >= 0 && s < B) start += am_valid_rows(state, stride, s, max_frames);
  }
  const int b = slots[j];
  const int mine = (b >= 0 && b < B) ? am_valid_rows(state, stride, b, max_frames) : 0;
  if (blockIdx.y == 0 && tid == 0) {
    if (j == 0) out_row0[0] = 0;
    out_row0[j + 1] = start + mine;
  }
  const int r_lo = blockIdx.y * AM_GATHER_ROWS;
  const int r_hi = min(min(mine, r_lo + AM_GATHER_ROWS), out_rows - start);   // rows the caller's buffer cannot hold stay unwritten
  if (r_lo >= r_hi) return;
  const float* rows = am_rows(state, stride, b);
  const int c4 = D >> 2, total = (r_hi - r_lo) * c4;
  for (int idx = tid; idx < total; idx += 256) {
    const int r = r_lo + idx / c4, c = idx % c4;
    stg4(out + (size_t)(start + r) * ldo + 4 * c, ldg4(rows + (size_t)r * D + 4 * c));
  }
}

}  // namespace
}  // namespace m3

using namespace m3;

extern "C" {

size_t m3_aed_memory_state_size(const m3_aed_memory_desc* desc) {
  if (check_memory_desc(desc)) return 0;
  return (size_t)desc->B * am_stride(desc);
}

int m3_aed_memory_reset(const m3_aed_memory_desc* desc, void* state, size_t state_bytes, m3_stream stream) {
  if (int rc = check_memory_state(desc, state, state_bytes, "aed_memory_reset")) return rc;
  if (desc->B == 0) return 0;
  hipLaunchKernelGGL(aed_memory_reset_kernel, dim3((unsigned)cdiv(desc->B, 256)), dim3(256), 0, (hipStream_t)stream, (char*)state,
                     am_stride(desc), desc->B, (const int32_t*)nullptr, 0);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_memory_reset_slots(const m3_aed_memory_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                              m3_stream stream) {
  if (int rc = check_memory_state(desc, state, state_bytes, "aed_memory_reset_slots")) return rc;
  M3_REQUIRE(n >= 0 && (n == 0 || slots != nullptr), "aed_memory_reset_slots: bad slot list (n = %d)", n);
  if (n == 0 || desc->B == 0) return 0;
  hipLaunchKernelGGL(aed_memory_reset_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (char*)state,
                     am_stride(desc), desc->B, slots, n);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_memory_append(const m3_aed_memory_desc* desc, void* state, size_t state_bytes, const float* x, int ldx, int T_chunk,
                         const int32_t* n_frames, m3_stream stream) {
  if (int rc = check_memory_state(desc, state, state_bytes, "aed_memory_append")) return rc;
  M3_REQUIRE(T_chunk >= 0 && T_chunk <= (1 << 14), "aed_memory_append: T_chunk = %d outside [0, 2^14]", T_chunk);
  M3_REQUIRE(ldx >= desc->D && (ldx & 3) == 0, "aed_memory_append: ldx = %d, need a multiple of 4 >= D = %d", ldx, desc->D);
  if (desc->B == 0 || T_chunk == 0) return 0;
  M3_REQUIRE(x != nullptr && n_frames != nullptr, "aed_memory_append: null pointer");
  M3_REQUIRE(((uintptr_t)x & 15) == 0, "aed_memory_append: x must be 16-byte aligned");
  hipLaunchKernelGGL(aed_memory_append_kernel, dim3((unsigned)desc->B), dim3(256), 0, (hipStream_t)stream, (char*)state, am_stride(desc),
                     desc->max_frames, desc->D, x, ldx, T_chunk, n_frames);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_memory_lengths(const m3_aed_memory_desc* desc, const void* state, size_t state_bytes, int32_t* len, m3_stream stream) {
  if (int rc = check_memory_state(desc, state, state_bytes, "aed_memory_lengths")) return rc;
  if (desc->B == 0) return 0;
  M3_REQUIRE(len != nullptr, "aed_memory_lengths: null pointer");
  hipLaunchKernelGGL(aed_memory_lengths_kernel, dim3((unsigned)cdiv(desc->B, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const char*)state, am_stride(desc), desc->B, desc->max_frames, len);
  M3_LAUNCH_CHECK();
  return 0;
}

int m3_aed_memory_gather(const m3_aed_memory_desc* desc, const void* state, size_t state_bytes, const int32_t* slots, int n,
                         float* out, int ldo, int out_rows, int32_t* out_row0, m3_stream stream) {
  if (int rc = check_memory_state(desc, state, state_bytes, "aed_memory_gather")) return rc;
  M3_REQUIRE(n >= 0 && n <= 65535 && (n == 0 || slots != nullptr), "aed_memory_gather: bad slot list (n = %d, at most 65535)", n);
  M3_REQUIRE((size_t)n * (size_t)desc->max_frames <= (size_t)INT_MAX, "aed_memory_gather: %d slots of %d frames overflow the int32 row offsets",
             n, desc->max_frames);
  M3_REQUIRE(out_row0 != nullptr && out_rows >= 0, "aed_memory_gather: out_row0 / out_rows = %d", out_rows);
  M3_REQUIRE(ldo >= desc->D && (ldo & 3) == 0, "aed_memory_gather: ldo = %d, need a multiple of 4 >= D = %d", ldo, desc->D);
  M3_REQUIRE(out_rows == 0 || (out != nullptr && ((uintptr_t)out & 15) == 0), "aed_memory_gather: out must be 16-byte aligned device memory");
  if (n == 0) {
    M3_CHECK_HIP(hipMemsetAsync(out_row0, 0, sizeof(int32_t), (hipStream_t)stream));
    return 0;
  }
  const int tiles = cdiv(desc->max_frames > 0 ? desc->max_frames : 1, AM_GATHER_ROWS);
  M3_REQUIRE(tiles <= 65535, "aed_memory_gather: max_frames = %d too large for the row-tile grid", desc->max_frames);
  hipLaunchKernelGGL(aed_memory_gather_kernel, dim3((unsigned)n, (unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const char*)state,
                     am_stride(desc), desc->B, desc->max_frames, desc->D, slots, out, ldo, out_rows, out_row0);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
