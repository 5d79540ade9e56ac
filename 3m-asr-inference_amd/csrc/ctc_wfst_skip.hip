// CTC blank-frame skipping in front of the graph search (include/m3asr.h "m3_wfst_skip"): which rows of a
// chunk of log-probabilities the token passing of ctc_wfst.hip has to see, chosen on the device and resumable at any frame
// boundary -- the last skipped row, the last best token and the map from decoded frames back to real ones live in
// caller-owned state.
//
//   device  wfst_skip_reset_kernel    the headers of the selected utterances
//           wfst_skip_select_kernel   one work-group per utterance and call: per tile of 64 frames (a) a wave per row computes
//                                     the blank test and the argmax into LDS, (b) one thread walks the rule over those flags
//                                     and lists the rows to emit, (c) every wave copies listed rows to their places
//           wfst_skip_map_kernel      word frames of the search (decoded frame numbers) -> real frame numbers, in place
//           wfst_skip_counts_kernel   frames seen / kept since the reset
//
// Nothing depends on thread order: (a) writes one flag pair per row, (b) is one thread, (c) copies disjoint rows.
#include <limits.h>
#include <math.h>

#include "../../include/m3asr.h"
#include "common.h"
#include "kernels.h"

namespace m3 {
namespace {

constexpr int kSkipThreads = 1024;          // 16 waves
constexpr int kSkipWaves = kSkipThreads / 64;
constexpr int kSkipTile = 64;               // frames whose flags sit in LDS at a time
constexpr int kSkipHdrWords = 8;
enum { SKIP_LAST_BLANK = 0, SKIP_LAST_BEST, SKIP_SAVED_FRAME, SKIP_SEEN, SKIP_KEPT };

struct SkipArgs {
  char* state;
  size_t per_utt;
  int B, V, blank, max_frames;
  float thresh;
  const int32_t* slots;
  const float* logp;
  int ld, T_chunk;
  const int32_t* n_frames;
  float* out;
  int ld_out;
  int32_t* n_kept;
};

size_t skip_per_utt(const m3_wfst_skip_desc* d) {
  return align_up((size_t)kSkipHdrWords * 4 + (size_t)d->V * 4 + (size_t)d->max_frames * 4, 16);
}

__device__ __forceinline__ int32_t* skip_hdr(const SkipArgs& a, int b) { return (int32_t*)(a.state + a.per_utt * (size_t)b); }
__device__ __forceinline__ float* skip_saved(const SkipArgs& a, int b) { return (float*)(skip_hdr(a, b) + kSkipHdrWords); }
__device__ __forceinline__ int32_t* skip_map(const SkipArgs& a, int b) { return (int32_t*)(skip_saved(a, b) + a.V); }

__global__ void wfst_skip_reset_kernel(SkipArgs a) {
  const int b = a.slots ? a.slots[blockIdx.x] : (int)blockIdx.x;
  if (b < 0 || b >= a.B || threadIdx.x >= kSkipHdrWords) return;
  skip_hdr(a, b)[threadIdx.x] = threadIdx.x == SKIP_LAST_BEST ? a.blank : 0;
}

__global__ __launch_bounds__(kSkipThreads) void wfst_skip_select_kernel(SkipArgs a) {
  __shared__ int s_skip[kSkipTile], s_best[kSkipTile];
  __shared__ int s_src[2 * kSkipTile], s_dst[2 * kSkipTile];   // the rows phase (c) copies: chunk frame (-1 = the state's row) -> row of out
  __shared__ int s_cnt, s_saved_src, s_last_blank;
  const int b = blockIdx.x;
  if (b >= a.B) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int32_t* hdr = skip_hdr(a, b);
  float* saved = skip_saved(a, b);
  int32_t* map = skip_map(a, b);
  const float* in = a.logp + (size_t)b * (size_t)a.T_chunk * (size_t)a.ld;
  float* out = a.out + (size_t)b * (size_t)(a.T_chunk + 1) * (size_t)a.ld_out;
  int n = a.n_frames[b];
  n = n < 0 ? 0 : (n > a.T_chunk ? a.T_chunk : n);
  // thread 0's copy of the header, the chunk frame of the saved row (-1: it is the state's) and the rows emitted by this call
  int last_blank = hdr[SKIP_LAST_BLANK] != 0, last_best = hdr[SKIP_LAST_BEST], saved_frame = hdr[SKIP_SAVED_FRAME];
  int seen = hdr[SKIP_SEEN], kept = hdr[SKIP_KEPT], saved_src = -1, emitted = 0;
  for (int t0 = 0; t0 < n; t0 += kSkipTile) {
    const int m = n - t0 < kSkipTile ? n - t0 : kSkipTile;
    // (a) a wave per row: the blank test, and the smallest index of the maximum (a NaN entry counts as -inf)
    for (int i = wave; i < m; i += kSkipWaves) {
      const float* row = in + (size_t)(t0 + i) * (size_t)a.ld;
      float val = -INFINITY;
      int idx = INT_MAX;
      for (int v = lane; v < a.V; v += 64) {
        float x = row[v];
        x = x != x ? -INFINITY : x;
        if (x > val || (x == val && v < idx)) { val = x; idx = v; }
      }
      for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(val, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
      }
      if (lane == 0) {
        s_skip[i] = row[a.blank] > a.thresh;
        s_best[i] = idx >= 0 && idx < a.V ? idx : 0;
      }
    }
    __syncthreads();
    // (b) the rule, serially over the tile's flags
    if (tid == 0) {
      int cnt = 0;
      for (int i = 0; i < m; ++i) {
        const int t = seen;
        if (seen < INT_MAX) ++seen;
        if (s_skip[i]) {
          last_blank = 1;
          saved_src = t0 + i;
          saved_frame = t;
          continue;
        }
        const int best = s_best[i];
        const int n_emit = best != a.blank && last_blank && best == last_best ? 2 : 1;
        for (int e = 2 - n_emit; e < 2; ++e) {      // e = 0: the saved row first, under its own frame number
          if (emitted <= a.T_chunk && cnt < 2 * kSkipTile) {
            s_src[cnt] = e == 0 ? saved_src : t0 + i;
            s_dst[cnt] = emitted;
            ++cnt;
            ++emitted;
          }
          if (kept >= 0 && kept < a.max_frames) map[kept] = e == 0 ? saved_frame : t;
          if (kept < INT_MAX) ++kept;
        }
        last_best = best;
        last_blank = 0;
      }
      s_cnt = cnt;
    }
    __syncthreads();
    // (c) every wave copies listed rows
    const int cnt = s_cnt;
    for (int e = wave; e < cnt; e += kSkipWaves) {
      const int src = s_src[e], dst = s_dst[e];
      if (src >= n || dst < 0 || dst > a.T_chunk) continue;
      const float* from = src < 0 ? saved : in + (size_t)src * (size_t)a.ld;
      float* to = out + (size_t)dst * (size_t)a.ld_out;
      for (int v = lane; v < a.V; v += 64) to[v] = from[v];
    }
    __syncthreads();
  }
  if (tid == 0) {
    s_saved_src = saved_src;
    s_last_blank = last_blank;
  }
  __syncthreads();
  // a chunk that ends skipped: its last skipped row goes into the state (every copy out of the state's row is done)
  const int src = s_saved_src;
  if (s_last_blank && src >= 0 && src < n) {
    const float* from = in + (size_t)src * (size_t)a.ld;
    for (int v = tid; v < a.V; v += kSkipThreads) saved[v] = from[v];
  }
  if (tid == 0) {
    hdr[SKIP_LAST_BLANK] = last_blank;
    hdr[SKIP_LAST_BEST] = last_best;
    hdr[SKIP_SAVED_FRAME] = saved_frame;
    hdr[SKIP_SEEN] = seen;
    hdr[SKIP_KEPT] = kept;
    a.n_kept[b] = emitted;
  }
}

__global__ void wfst_skip_map_kernel(SkipArgs a, int32_t* frames, int ld_frames, const int32_t* n_words) {
  const int b = blockIdx.x;
  if (b >= a.B) return;
  int n = n_words[b];
  n = n > ld_frames ? ld_frames : n;
  const int32_t* hdr = skip_hdr(a, b);
  const int32_t* map = skip_map(a, b);
  const int seen = hdr[SKIP_SEEN], kept = hdr[SKIP_KEPT];
  const int held = kept < a.max_frames ? kept : a.max_frames;
  int32_t* f = frames + (size_t)b * (size_t)ld_frames;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int r = f[i];
    f[i] = r >= 0 && r < held ? map[r] : seen;
  }
}

__global__ void wfst_skip_counts_kernel(SkipArgs a, int32_t* seen, int32_t* kept) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  seen[b] = skip_hdr(a, b)[SKIP_SEEN];
  kept[b] = skip_hdr(a, b)[SKIP_KEPT];
}

int skip_check_desc(const m3_wfst_skip_desc* d, const char* who) {
  M3_REQUIRE(d != nullptr, "%s: null descriptor", who);
  M3_REQUIRE(d->B >= 0 && d->B <= 32768, "%s: B = %d outside [0, 32768]", who, d->B);
  M3_REQUIRE(d->V >= 1 && d->V <= (1 << 24), "%s: V = %d outside [1, 2^24]", who, d->V);
  M3_REQUIRE(d->blank >= 0 && d->blank < d->V, "%s: blank = %d outside [0, %d)", who, d->blank, d->V);
  M3_REQUIRE(d->max_frames >= 0 && d->max_frames <= (1 << 28), "%s: max_frames = %d outside [0, 2^28]", who, d->max_frames);
  M3_REQUIRE(!std::isnan(d->log_blank_thresh), "%s: log_blank_thresh is NaN", who);
  return 0;
}

int skip_fill_args(const m3_wfst_skip_desc* d, const void* state, size_t bytes, const char* who, SkipArgs* a) {
  if (int rc = skip_check_desc(d, who)) return rc;
  const size_t per = skip_per_utt(d);
  M3_REQUIRE(state != nullptr && ((uintptr_t)state & 15) == 0, "%s: state is null or not 16-byte aligned", who);
  M3_REQUIRE(bytes >= per * (size_t)d->B, "%s: state of %zu bytes < %zu", who, bytes, per * (size_t)d->B);
  *a = SkipArgs{};
  a->state = (char*)const_cast<void*>(state);
  a->per_utt = per;
  a->B = d->B;
  a->V = d->V;
  a->blank = d->blank;
  a->max_frames = d->max_frames;
  a->thresh = d->log_blank_thresh;
  return 0;
}

}  // namespace

size_t wfst_skip_state_size(const m3_wfst_skip_desc* d) {
  if (skip_check_desc(d, "wfst_skip_state_size")) return 0;
  return skip_per_utt(d) * (size_t)d->B;
}

int launch_wfst_skip_reset(const m3_wfst_skip_desc* d, void* state, size_t bytes, const int32_t* slots, int n, hipStream_t stream) {
  SkipArgs a;
  if (int rc = skip_fill_args(d, state, bytes, "wfst_skip_reset", &a)) return rc;
  M3_REQUIRE(n >= 0 && n <= d->B, "wfst_skip_reset: %d slots for B = %d", n, d->B);
  const int count = slots ? n : d->B;
  if (count == 0) return 0;
  a.slots = slots;                                               // (a slot outside [0, B) is skipped)
  hipLaunchKernelGGL(wfst_skip_reset_kernel, dim3(count), dim3(64), 0, stream, a);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_wfst_skip_select(const m3_wfst_skip_desc* d, void* state, size_t bytes, const float* logp, int ld, int T_chunk,
                            const int32_t* n_frames, float* out, int ld_out, int32_t* n_kept, hipStream_t stream) {
  SkipArgs a;
  if (int rc = skip_fill_args(d, state, bytes, "wfst_skip_select", &a)) return rc;
  M3_REQUIRE(T_chunk >= 0 && T_chunk < INT_MAX, "wfst_skip_select: T_chunk = %d < 0", T_chunk);
  M3_REQUIRE(ld >= d->V, "wfst_skip_select: ld = %d < V = %d", ld, d->V);
  M3_REQUIRE(ld_out >= d->V, "wfst_skip_select: ld_out = %d < V = %d", ld_out, d->V);
  M3_REQUIRE(n_frames != nullptr && out != nullptr && n_kept != nullptr && (logp != nullptr || T_chunk == 0),
             "wfst_skip_select: null pointer");
  if (d->B == 0) return 0;
  a.logp = logp;
  a.ld = ld;
  a.T_chunk = T_chunk;
  a.n_frames = n_frames;
  a.out = out;
  a.ld_out = ld_out;
  a.n_kept = n_kept;
  hipLaunchKernelGGL(wfst_skip_select_kernel, dim3(d->B), dim3(kSkipThreads), 0, stream, a);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_wfst_skip_map_frames(const m3_wfst_skip_desc* d, const void* state, size_t bytes, int32_t* frames, int ld_frames,
                                const int32_t* n_words, hipStream_t stream) {
  SkipArgs a;
  if (int rc = skip_fill_args(d, state, bytes, "wfst_skip_map_frames", &a)) return rc;
  M3_REQUIRE(ld_frames >= 0, "wfst_skip_map_frames: ld_frames = %d < 0", ld_frames);
  M3_REQUIRE(frames != nullptr && n_words != nullptr, "wfst_skip_map_frames: null pointer");
  if (d->B == 0 || ld_frames == 0) return 0;
  hipLaunchKernelGGL(wfst_skip_map_kernel, dim3(d->B), dim3(256), 0, stream, a, frames, ld_frames, n_words);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_wfst_skip_counts(const m3_wfst_skip_desc* d, const void* state, size_t bytes, int32_t* seen, int32_t* kept,
                            hipStream_t stream) {
  SkipArgs a;
  if (int rc = skip_fill_args(d, state, bytes, "wfst_skip_counts", &a)) return rc;
  M3_REQUIRE(seen != nullptr && kept != nullptr, "wfst_skip_counts: null pointer");
  if (d->B == 0) return 0;
  hipLaunchKernelGGL(wfst_skip_counts_kernel, dim3(grid1d((size_t)d->B, 1024)), dim3(256), 0, stream, a, seen, kept);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
