// Long recordings in: Kaldi's compute-vad on the device, a segmenter on its flags, and the cut of feature rows
// into an engine batch -- the step between the features and a full-context encoder whose positional table ends at max_len.
//
// Four launches, each on a ragged batch with device length vectors; no result depends on B, T or the launch geometry.
//
// (a) vad_log_energy_kernel.  The framing of fbank.hip (400 samples every 160, snip_edges, one wave64 per frame, four frames per
//     work-group), so frame k here is frame k of the features.  The frame's samples go to LDS as float, whatever they were, and
//     lane l then owns samples l, l + 64, ..: mean = wave_sum(partial sums) / 400, E = wave_sum(partial sums of (x - mean)^2),
//     log(max(E, FLT_EPSILON)) -- Kaldi's raw energy, after DC removal, before pre-emphasis and window.  One lane order for int16
//     and float32 input: the same bits.
// (b) vad_decide_kernel.  Kaldi's ComputeVadEnergy.  A work-group owns VD_TILE consecutive frames of one row.  Every work-group
//     of a row adds up the WHOLE row for the threshold (float64; lane l takes frames l, l + 256, .., then a fixed tree): the row
//     comes out of L2, the order is a function of the row alone, and the launch needs no second pass or workspace.  The pass is
//     skipped when energy_mean_scale == 0.  The tile's "logE > threshold" bits and VAD_MAX_CONTEXT frames of halo either side
//     go to LDS as bytes; a frame counts its window there and compares in fp32 as Kaldi does.
// (c) vad_segments_kernel.  One wave64 per row, streaming it SG_UNROLL * 64 frames at a time -- nothing of the row is kept, so
//     its length is bounded by T alone.  A ballot turns 64 flags into a mask; its rises and falls are walked in order by uniform
//     control flow that holds the open run [run_s, run_e): a rise closer than min_silence to run_e continues it (close), any
//     other rise finishes it.  A finished run shorter than min_speech is dropped (open), the others are padded and, while
//     longer than max_segment, cut at the lowest logE of the search window: a lane-parallel arg-min on (value, index), the
//     lower index on a tie.  Segments leave in ascending order; lane 0 writes the first `capacity` and the count is always true.
// (d) segment_gather_kernel.  Features are computed ONCE over the whole recording and then cut, so a segment's delta columns
//     at its edges come from the real neighbouring frames, not from a replicated edge: the deliberate difference from
//     featurising cut audio.  A work-group owns GA_TILE destination frames of one job and copies (frame, column quad) items
//     with 16-byte accesses, or (frame, column) items when a stride, a pointer or cols is not a whole 16 bytes; frames behind
//     the segment are zeros, columns >= cols are not touched.
#include <float.h>
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace m3 {

namespace {

constexpr int LE_FRAME = 400, LE_SHIFT = 160, LE_WAVES = 4;

template <bool INT16>
__global__ __launch_bounds__(64 * LE_WAVES) void vad_log_energy_kernel(const void* __restrict__ pcm, long ld_pcm,
                                                                       const int32_t* __restrict__ n_samples, int B, int T,
                                                                       float* __restrict__ out, long ld_out,
                                                                       int32_t* __restrict__ len_out, float log_floor) {
  __shared__ __attribute__((aligned(16))) float s_x[LE_WAVES][LE_FRAME];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * LE_WAVES + wave;
  const bool in_range = f < (long)B * T;
  const int b = in_range ? (int)(f / T) : 0, t = in_range ? (int)(f % T) : 0;
  int len = 0;
  if (in_range) {
    long n = n_samples[b];
    n = n < 0 ? 0 : (n > ld_pcm ? ld_pcm : n);        // a row holds ld_pcm samples at most
    len = n < LE_FRAME ? 0 : 1 + (int)((n - LE_FRAME) / LE_SHIFT);
    len = len < T ? len : T;
    if (t == 0 && lane == 0) len_out[b] = len;
  }
  const bool live = in_range && t < len;
  float* const xs = s_x[wave];
  if (live) {                                         // 160 t + 400 <= n <= ld_pcm: the frame lies inside the row
    const long first = (long)b * ld_pcm + (long)LE_SHIFT * t;
    if (INT16) {
      if (lane < LE_FRAME / 8) {
        const u32x4 v = ldg16b(reinterpret_cast<const int16_t*>(pcm) + first + 8 * lane);
        f32x4 lo, hi;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          lo[2 * j] = (float)(int16_t)(v[j] & 0xffffu);
          lo[2 * j + 1] = (float)(int16_t)(v[j] >> 16);
          hi[2 * j] = (float)(int16_t)(v[2 + j] & 0xffffu);
          hi[2 * j + 1] = (float)(int16_t)(v[2 + j] >> 16);
        }
        *reinterpret_cast<f32x4*>(xs + 8 * lane) = lo;
        *reinterpret_cast<f32x4*>(xs + 8 * lane + 4) = hi;
      }
    } else {
      for (int c = lane; c < LE_FRAME / 4; c += 64)
        *reinterpret_cast<f32x4*>(xs + 4 * c) = ldg4(reinterpret_cast<const float*>(pcm) + first + 4 * c);
    }
  }
  __syncthreads();
  if (live) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const int i = lane + 64 * r;
      if (i < LE_FRAME) s += xs[i];
    }
    const float mean = wave_sum(s) / (float)LE_FRAME;
    float e = 0.f;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const int i = lane + 64 * r;
      if (i < LE_FRAME) {
        const float d = xs[i] - mean;
        e += d * d;
      }
    }
    e = wave_sum(e);
    if (lane == 0) out[(long)b * ld_out + t] = e <= FLT_EPSILON ? log_floor : logf(e);
  } else if (in_range && lane == 0) {
    out[(long)b * ld_out + t] = 0.f;                  // behind the row's last frame: zeros
  }
}

constexpr int VD_THREADS = 256, VD_TILE = 4096, VD_HALO = VAD_MAX_CONTEXT;

__global__ __launch_bounds__(VD_THREADS) void vad_decide_kernel(const float* __restrict__ logE, long ld_e,
                                                                const int32_t* __restrict__ lens, int T, float energy_threshold,
                                                                float mean_scale, int context, float proportion,
                                                                uint8_t* __restrict__ flags, long ld_flags,
                                                                float* __restrict__ threshold_out) {
  __shared__ double s_sum[VD_THREADS];
  __shared__ uint8_t s_above[VD_TILE + 2 * VD_HALO];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile0 = blockIdx.x * VD_TILE;             // < T
  const int len = min(max(lens[b], 0), T);
  const float* const row = logE + (long)b * ld_e;
  double mean = 0.0;
  if (mean_scale != 0.f && len > 0) {
    double s = 0.0;
    for (int i = tid; i < len; i += VD_THREADS) s += (double)row[i];
    s_sum[tid] = s;
    __syncthreads();
    for (int w = VD_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) s_sum[tid] += s_sum[tid + w];
      __syncthreads();
    }
    mean = s_sum[0] / (double)len;
  }
  const float thr = (float)((double)energy_threshold + (double)mean_scale * mean);
  if (blockIdx.x == 0 && tid == 0) threshold_out[b] = thr;
  for (int i = tid; i < VD_TILE + 2 * VD_HALO; i += VD_THREADS) {
    const long t = (long)tile0 - VD_HALO + i;
    s_above[i] = (t >= 0 && t < len && row[t] > thr) ? 1 : 0;
  }
  __syncthreads();
  const int tile_n = min(VD_TILE, T - tile0);
  uint8_t* const frow = flags + (long)b * ld_flags + tile0;
  for (int i = tid; i < tile_n; i += VD_THREADS) {
    const int t = tile0 + i;
    uint8_t v = 0;
    if (t < len) {
      const int lo = max(t - context, 0), hi = min(t + context, len - 1);   // |lo - t|, |hi - t| <= context <= VD_HALO
      int num = 0;
      for (int u = lo; u <= hi; ++u) num += s_above[u - tile0 + VD_HALO];
      v = (float)num >= (float)(hi - lo + 1) * proportion ? 1 : 0;
    }
    frow[i] = v;
  }
}

constexpr int SG_UNROLL = 8;

struct SegArgs {
  const uint8_t* flags;
  long ld_flags;
  const float* logE;
  long ld_e;
  const int32_t* lens;
  int T, min_silence, min_speech, pad, max_segment, split_search;
  int32_t* segments;
  int capacity;
  int32_t* n_segments;
};

// the open run [s, e) is finished: open, pad, split.  Uniform over the wave; returns the new segment count.
__device__ __forceinline__ int seg_finish(const SegArgs& a, const float* __restrict__ erow, int32_t* __restrict__ seg, int len,
                                          int s, int e, int count, int lane) {
  if (e - s < a.min_speech) return count;
  s = max(s - a.pad, 0);
  e = min(e + a.pad, len);
  while (e - s > a.max_segment) {
    const int w0 = s + a.max_segment - a.split_search, w1 = s + a.max_segment;   // s < w0 < w1 < e <= len
    float best_v = INFINITY;
    int best_i = 0x7fffffff;
    for (int i = w0 + lane; i < w1; i += 64) {        // ascending per lane: `<` keeps the lowest index of equal values
      const float v = erow[i];
      if (v < best_v || best_i == 0x7fffffff) {
        best_v = v;
        best_i = i;
      }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const float ov = __shfl_xor(best_v, m, 64);
      const int oi = __shfl_xor(best_i, m, 64);
      if (oi != 0x7fffffff && (best_i == 0x7fffffff || ov < best_v || (ov == best_v && oi < best_i))) {
        best_v = ov;
        best_i = oi;
      }
    }
    int cut = __builtin_amdgcn_readfirstlane(best_i);
    if (cut < w0 || cut >= w1) cut = w0;              // values that do not order (NaN): any frame of the window, never outside it
    if (count < a.capacity && lane == 0) {
      seg[2 * count] = s;
      seg[2 * count + 1] = cut;
    }
    ++count;
    s = cut;
  }
  if (count < a.capacity && lane == 0) {
    seg[2 * count] = s;
    seg[2 * count + 1] = e;
  }
  return count + 1;
}

__global__ __launch_bounds__(64) void vad_segments_kernel(const SegArgs a) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const int len = min(max(a.lens[b], 0), a.T);
  const uint8_t* const frow = a.flags + (long)b * a.ld_flags;
  const float* const erow = a.logE + (long)b * a.ld_e;
  int32_t* const seg = a.segments + (long)b * a.capacity * 2;
  int count = 0, run_s = -1, run_e = -1;              // the open run, closed so far: [run_s, run_e); none while run_s < 0
  unsigned long long prev = 0;                        // the flag of the frame before the current word
  for (long base = 0; base < len; base += 64 * SG_UNROLL) {
    unsigned long long words[SG_UNROLL];
#pragma unroll
    for (int j = 0; j < SG_UNROLL; ++j) {
      const long t = base + 64 * j + lane;
      const bool on = t < len && frow[t] != 0;
      words[j] = __ballot(on);
    }
#pragma unroll
    for (int j = 0; j < SG_UNROLL; ++j) {
      const unsigned long long m = words[j], before = (m << 1) | prev;
      unsigned long long edges = m ^ before;          // bit i: frame i differs from the frame before it
      prev = m >> 63;
      const int t0 = (int)(base + 64 * j);
      while (edges) {
        const int bit = __builtin_ctzll(edges);
        edges &= edges - 1;
        const int t = t0 + bit;
        if ((m >> bit) & 1ull) {                      // a rise
          if (run_s >= 0 && t - run_e >= a.min_silence) {
            count = seg_finish(a, erow, seg, len, run_s, run_e, count, lane);
            run_s = -1;
          }
          if (run_s < 0) run_s = t;
        } else {                                      // a fall: the voiced run ended in front of t
          run_e = t;
        }
      }
    }
  }
  if (prev) run_e = len;                              // voiced up to the row's end
  if (run_s >= 0) count = seg_finish(a, erow, seg, len, run_s, run_e, count, lane);
  if (lane == 0) a.n_segments[b] = count;
}

constexpr int GA_THREADS = 256, GA_TILE = 32;

template <bool VEC>
__global__ __launch_bounds__(GA_THREADS) void segment_gather_kernel(const float* __restrict__ src, long ld_src, int T_all,
                                                                    const int32_t* __restrict__ jobs, int T_max, int cols,
                                                                    float* __restrict__ dst, long ld_dst, long bs_dst,
                                                                    int32_t* __restrict__ len_out) {
  constexpr int E = VEC ? 4 : 1;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile0 = blockIdx.x * GA_TILE;             // < T_max
  const int tile_n = min(GA_TILE, T_max - tile0);
  const long first = (long)jobs[3 * b] + (long)jobs[3 * b + 1];
  long n = (long)jobs[3 * b + 2] - (long)jobs[3 * b + 1];
  n = n < T_max ? n : T_max;
  if (first < 0 || first >= T_all) n = 0;             // a job that leaves the matrix is cut short where it leaves
  n = n < (long)T_all - first ? n : (long)T_all - first;
  n = n < 0 ? 0 : n;
  if (blockIdx.x == 0 && tid == 0) len_out[b] = (int)n;
  const int Q = VEC ? cols / 4 : cols;
  float* const orow = dst + (long)b * bs_dst + (long)tile0 * ld_dst;
  for (int i = tid; i < tile_n * Q; i += GA_THREADS) {
    const int t = i / Q, q = i - t * Q;
    float* const o = orow + (long)t * ld_dst + q * E;
    const bool real = tile0 + t < n;
    const float* const p = src + (first + tile0 + t) * ld_src + q * E;   // read only when real: then first + tile0 + t < T_all
    if (VEC)
      stg4(o, real ? ldg4(p) : f32x4{0.f, 0.f, 0.f, 0.f});
    else
      *o = real ? *p : 0.f;
  }
}

}  // namespace

int vad_options_ok(float energy_mean_scale, int context, float proportion_threshold) {
  M3_REQUIRE(context >= 0 && context <= VAD_MAX_CONTEXT, "vad: context=%d outside [0, %d]", context, VAD_MAX_CONTEXT);
  M3_REQUIRE(proportion_threshold > 0.f && proportion_threshold < 1.f, "vad: proportion_threshold=%g outside (0, 1)", proportion_threshold);
  M3_REQUIRE(energy_mean_scale >= 0.f && energy_mean_scale <= FLT_MAX, "vad: energy_mean_scale=%g is negative or not finite",
             energy_mean_scale);
  return 0;
}

int segment_options_ok(int min_silence, int min_speech, int pad, int max_segment, int split_search) {
  M3_REQUIRE(min_silence >= 0 && pad >= 0, "segments: min_silence=%d or pad=%d is negative", min_silence, pad);
  M3_REQUIRE(min_speech >= 7, "segments: min_speech=%d is below 7 frames (the encoder's shortest input)", min_speech);
  M3_REQUIRE(2L * pad <= min_silence, "segments: 2 * pad=%ld exceeds min_silence=%d (padded runs could touch)", 2L * pad, min_silence);
  M3_REQUIRE(split_search >= 1 && (long)split_search <= (long)max_segment - 7,
             "segments: split_search=%d outside [1, max_segment - 7 = %ld]", split_search, (long)max_segment - 7);
  return 0;
}

int launch_vad_log_energy(const void* pcm, int pcm_is_int16, long ld_pcm, const int32_t* n_samples, int B, int T, float* log_energy,
                          long ld_out, int32_t* len_out, hipStream_t stream) {
  const long frames = (long)B * T;
  if (frames == 0) return 0;
  M3_REQUIRE(frames < (1L << 26), "vad_log_energy: B * T = %ld frames, one launch takes fewer than 2^26 (one wave each)", frames);
  const unsigned grid = (unsigned)((frames + LE_WAVES - 1) / LE_WAVES);
  const float log_floor = (float)log((double)FLT_EPSILON);
  if (pcm_is_int16)
    hipLaunchKernelGGL(vad_log_energy_kernel<true>, dim3(grid), dim3(64 * LE_WAVES), 0, stream, pcm, ld_pcm, n_samples, B, T,
                       log_energy, ld_out, len_out, log_floor);
  else
    hipLaunchKernelGGL(vad_log_energy_kernel<false>, dim3(grid), dim3(64 * LE_WAVES), 0, stream, pcm, ld_pcm, n_samples, B, T,
                       log_energy, ld_out, len_out, log_floor);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_vad_decide(const float* log_energy, long ld_e, const int32_t* lens, int B, int T, float energy_threshold,
                      float energy_mean_scale, int context, float proportion_threshold, uint8_t* flags, long ld_flags,
                      float* threshold_out, hipStream_t stream) {
  if (int rc = vad_options_ok(energy_mean_scale, context, proportion_threshold)) return rc;
  if (B == 0 || T == 0) return 0;
  const dim3 grid((unsigned)((T + VD_TILE - 1) / VD_TILE), (unsigned)B);
  hipLaunchKernelGGL(vad_decide_kernel, grid, dim3(VD_THREADS), 0, stream, log_energy, ld_e, lens, T, energy_threshold,
                     energy_mean_scale, context, proportion_threshold, flags, ld_flags, threshold_out);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_vad_segments(const uint8_t* flags, long ld_flags, const float* log_energy, long ld_e, const int32_t* lens, int B, int T,
                        int min_silence, int min_speech, int pad, int max_segment, int split_search, int32_t* segments,
                        int capacity, int32_t* n_segments, hipStream_t stream) {
  if (int rc = segment_options_ok(min_silence, min_speech, pad, max_segment, split_search)) return rc;
  if (B == 0 || T == 0) return 0;
  SegArgs a;
  a.flags = flags;
  a.ld_flags = ld_flags;
  a.logE = log_energy;
  a.ld_e = ld_e;
  a.lens = lens;
  a.T = T;
  a.min_silence = min_silence;
  a.min_speech = min_speech;
  a.pad = pad;
  a.max_segment = max_segment;
  a.split_search = split_search;
  a.segments = segments;
  a.capacity = capacity;
  a.n_segments = n_segments;
  hipLaunchKernelGGL(vad_segments_kernel, dim3((unsigned)B), dim3(64), 0, stream, a);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_segment_gather(const float* src, long ld_src, int T_all, const int32_t* jobs, int B, int T_max, int cols, float* dst,
                          long ld_dst, long bs_dst, int32_t* len_out, hipStream_t stream) {
  if (B == 0 || T_max == 0) return 0;
  const dim3 grid((unsigned)((T_max + GA_TILE - 1) / GA_TILE), (unsigned)B);
  const bool vec = cols % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && bs_dst % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(segment_gather_kernel<true>, grid, dim3(GA_THREADS), 0, stream, src, ld_src, T_all, jobs, T_max, cols, dst,
                       ld_dst, bs_dst, len_out);
  else
    hipLaunchKernelGGL(segment_gather_kernel<false>, grid, dim3(GA_THREADS), 0, stream, src, ld_src, T_all, jobs, T_max, cols, dst,
                       ld_dst, bs_dst, len_out);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
