// Kaldi-style log-Mel filter bank on the device: samples -> the feature frames the encoder was trained on.
//
// Contract (compute-fbank-feats with the options of a served model): 16 kHz mono PCM in the int16 value range, frames of 400
// samples every 160 (snip_edges), per frame: subtract the mean, pre-emphasis 0.97, Povey window, zero-pad to 512, power
// spectrum of bins 0..255, triangular mel filters with weights taken in the mel domain, log(max(E, FLT_EPSILON)).  No dither,
// no energy column, no CMVN.
//
// Layout: one wave64 per frame, four frames per work-group.  The 512-point real FFT runs as a 256-point complex FFT of
// z[n] = x[2n] + i x[2n+1]: four radix-4 Stockham stages, one butterfly (4 points) per lane and stage, exchanged through two
// 2 KiB LDS buffers per wave, then the real-input post-pass into 256 powers that stay in LDS; every mel bin sums its own
// contiguous range of powers in ascending order.  Twiddles, window and mel weights are tables built on the HOST in float64
// and rounded once (fbank_tables_build): the kernel calls no sincos / pow, only logf.  A frame is computed by its wave alone,
// from its 400 samples, in a lane layout that does not depend on B, T or the frame's place in the grid, so its bits do not
// either.
#include <float.h>
#include <math.h>
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace m3 {

namespace {

constexpr int FB_FRAME = 400, FB_SHIFT = 160, FB_HALF = 256, FB_WAVES = 4, FB_MAX_BINS = 128, FB_MAX_W = 512;

// The device image of the tables.  tw256[q] = exp(-2 pi i q / 256) (FFT twiddles), tw512[k] = exp(-2 pi i k / 512) (real-input
// post-pass), mel bin m sums power[mel_lo[m] + i] * mel_w[mel_off[m] + i] for i < mel_n[m].
struct FbankTables {
  int32_t num_bins;
  float log_floor;                      // log(FLT_EPSILON), rounded on the host
  int32_t reserved[2];
  float tw256[FB_HALF][2];
  float tw512[FB_HALF][2];
  float window[FB_FRAME];
  int32_t mel_lo[FB_MAX_BINS], mel_n[FB_MAX_BINS], mel_off[FB_MAX_BINS];
  float mel_w[FB_MAX_W];
};
static_assert(sizeof(FbankTables) % 16 == 0, "the table image is read with 16-byte alignment");

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// one radix-4 butterfly on twiddled inputs; results to out[j + r P]
template <int P>
__device__ __forceinline__ void radix4_store(float2 u0, float2 u1, float2 u2, float2 u3, float2* __restrict__ out, int lane) {
  const int k = lane & (P - 1), j = ((lane - k) << 2) + k;
  const float2 v0 = make_float2(u0.x + u2.x, u0.y + u2.y), v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
  const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y), v3 = make_float2(u1.y - u3.y, u3.x - u1.x);   // -i (u1 - u3)
  out[j] = make_float2(v0.x + v2.x, v0.y + v2.y);
  out[j + P] = make_float2(v1.x + v3.x, v1.y + v3.y);
  out[j + 2 * P] = make_float2(v0.x - v2.x, v0.y - v2.y);
  out[j + 3 * P] = make_float2(v1.x - v3.x, v1.y - v3.y);
}
// Stockham stage with sub-transform length P (4, 16, 64): lane reads in[lane + 64 r], twiddles by exp(-2 pi i r k / (4 P))
template <int P>
__device__ __forceinline__ void radix4_stage(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw, int lane) {
  const int q = (lane & (P - 1)) * (64 / P);
  radix4_store<P>(in[lane], cmul(tw[q], in[lane + 64]), cmul(tw[2 * q], in[lane + 128]), cmul(tw[3 * q], in[lane + 192]), out, lane);
}

template <bool INT16>
__global__ __launch_bounds__(64 * FB_WAVES) void fbank_kernel(const FbankTables* __restrict__ tab, const void* __restrict__ pcm,
                                                              long ld_pcm, const int32_t* __restrict__ n_samples, int B, int T,
                                                              int nbins, float* __restrict__ feat, long ld_feat,
                                                              int32_t* __restrict__ feat_len) {
  __shared__ float2 s_tw[2 * FB_HALF];                 // tw256 then tw512
  __shared__ float2 s_buf[FB_WAVES][2][FB_HALF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * FB_WAVES + wave;
  const bool in_range = f < (long)B * T;
  const int b = in_range ? (int)(f / T) : 0, t = in_range ? (int)(f % T) : 0;
  int len = 0;
  if (in_range) {
    long n = n_samples[b];
    n = n < 0 ? 0 : (n > ld_pcm ? ld_pcm : n);        // a row holds ld_pcm samples at most
    len = n < FB_FRAME ? 0 : 1 + (int)((n - FB_FRAME) / FB_SHIFT);
    len = len < T ? len : T;
    if (t == 0 && lane == 0) feat_len[b] = len;
  }
  const bool live = in_range && t < len;
  float* const row = feat + (in_range ? ((long)b * T + t) * ld_feat : 0);
  if (in_range && !live)                               // behind the utterance's last frame: zeros
    for (int m = lane; m < nbins; m += 64) row[m] = 0.f;
  if (!__syncthreads_or(live)) return;

  for (int i = threadIdx.x; i < 2 * FB_HALF; i += 64 * FB_WAVES) s_tw[i] = reinterpret_cast<const float2*>(&tab->tw256[0][0])[i];
  float2* const bufA = s_buf[wave][0];
  float2* const bufB = s_buf[wave][1];
  float* const xs = reinterpret_cast<float*>(bufB);    // the frame's samples as float (1600 of bufB's 2048 bytes)
  if (live) {
    const long first = (long)b * ld_pcm + (long)FB_SHIFT * t;
    if (INT16) {
      if (lane < FB_FRAME / 8) {
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
      for (int c = lane; c < FB_FRAME / 4; c += 64)
        *reinterpret_cast<f32x4*>(xs + 4 * c) = ldg4(reinterpret_cast<const float*>(pcm) + first + 4 * c);
    }
  }
  __syncthreads();
  if (live) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const int i = lane + 64 * r;
      if (i < FB_FRAME) s += xs[i];
    }
    const float mean = wave_sum(s) / (float)FB_FRAME;
    // DC removal, pre-emphasis and window on the way into the first stage: z[n] = y[2n] + i y[2n+1], zero behind n = 199
    float2 u[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = lane + 64 * r;
      u[r] = make_float2(0.f, 0.f);
      if (n < FB_FRAME / 2) {
        const float x0 = xs[2 * n] - mean, x1 = xs[2 * n + 1] - mean;
        const float xm = n == 0 ? x0 : xs[2 * n - 1] - mean;
        const float2 w = reinterpret_cast<const float2*>(tab->window)[n];
        u[r] = make_float2((x0 - 0.97f * xm) * w.x, (x1 - 0.97f * x0) * w.y);
      }
    }
    radix4_store<1>(u[0], u[1], u[2], u[3], bufA, lane);
  }
  __syncthreads();
  if (live) radix4_stage<4>(bufA, bufB, s_tw, lane);
  __syncthreads();
  if (live) radix4_stage<16>(bufB, bufA, s_tw, lane);
  __syncthreads();
  if (live) radix4_stage<64>(bufA, bufB, s_tw, lane);
  __syncthreads();
  float* const pw = reinterpret_cast<float*>(bufA);
  if (live) {
    // real-input post-pass: X[k] = (Z[k] + conj Z[256-k]) / 2 + exp(-2 pi i k / 512) (Z[k] - conj Z[256-k]) / (2 i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = lane + 64 * r;
      const float2 z = bufB[k], y = bufB[(FB_HALF - k) & (FB_HALF - 1)], w = s_tw[FB_HALF + k];
      const float er = 0.5f * (z.x + y.x), ei = 0.5f * (z.y - y.y);
      const float orr = 0.5f * (z.y + y.y), oi = -0.5f * (z.x - y.x);
      const float re = er + (w.x * orr - w.y * oi), im = ei + (w.x * oi + w.y * orr);
      pw[k] = re * re + im * im;
    }
  }
  __syncthreads();
  if (live) {
    for (int m = lane; m < nbins; m += 64) {
      int lo = tab->mel_lo[m], n = tab->mel_n[m], off = tab->mel_off[m];
      lo = min(max(lo, 0), FB_HALF);                   // a table that is not one of ours must not become an address
      n = min(max(n, 0), FB_HALF - lo);
      off = min(max(off, 0), FB_MAX_W - n);
      float e = 0.f;
      for (int i = 0; i < n; ++i) e += pw[lo + i] * tab->mel_w[off + i];
      row[m] = e <= FLT_EPSILON ? tab->log_floor : logf(e);
    }
  }
}

double mel_of(double f) { return 1127.0 * log(1.0 + f / 700.0); }

}  // namespace

size_t fbank_tables_bytes() { return sizeof(FbankTables); }

// The tables in float64, rounded once to float32, into a host image of fbank_tables_bytes() bytes.
int fbank_tables_build(int num_mel_bins, double sample_rate, double low_freq, double high_freq, void* host_image) {
  FbankTables* t = reinterpret_cast<FbankTables*>(host_image);
  memset(t, 0, sizeof(FbankTables));
  const double pi = 3.14159265358979323846;
  t->num_bins = num_mel_bins;
  t->log_floor = (float)log((double)FLT_EPSILON);
  for (int q = 0; q < FB_HALF; ++q) {
    t->tw256[q][0] = (float)cos(2.0 * pi * q / 256.0);
    t->tw256[q][1] = (float)-sin(2.0 * pi * q / 256.0);
    t->tw512[q][0] = (float)cos(2.0 * pi * q / 512.0);
    t->tw512[q][1] = (float)-sin(2.0 * pi * q / 512.0);
  }
  for (int i = 0; i < FB_FRAME; ++i) t->window[i] = (float)pow(0.5 - 0.5 * cos(2.0 * pi * i / (FB_FRAME - 1)), 0.85);
  const double mel_low = mel_of(low_freq), mel_high = mel_of(high_freq), delta = (mel_high - mel_low) / (num_mel_bins + 1);
  int used = 0;
  for (int m = 0; m < num_mel_bins; ++m) {
    const double left = mel_low + m * delta, centre = left + delta, right = centre + delta;
    int lo = -1, n = 0;
    for (int j = 0; j < FB_HALF; ++j) {
      const double mj = mel_of(j * sample_rate / (2.0 * FB_HALF));
      if (mj > left && mj < right) {                  // both edges open
        if (lo < 0) lo = j;
        if (used + n >= FB_MAX_W) {
          set_error("fbank tables: more than %d mel weights", FB_MAX_W);
          return -2;
        }
        t->mel_w[used + n++] = (float)(mj <= centre ? (mj - left) / (centre - left) : (right - mj) / (right - centre));
      }
    }
    t->mel_lo[m] = lo < 0 ? 0 : lo;
    t->mel_n[m] = n;
    t->mel_off[m] = used;
    used += n;
  }
  return 0;
}

int launch_fbank(const void* tables, const void* pcm, int pcm_is_int16, int ld_pcm, const int32_t* n_samples, int B, int T,
                 int num_mel_bins, float* feat, int ld_feat, int32_t* feat_len, hipStream_t stream) {
  const long frames = (long)B * T;
  if (frames == 0) return 0;
  const unsigned grid = (unsigned)((frames + FB_WAVES - 1) / FB_WAVES);
  const FbankTables* tab = reinterpret_cast<const FbankTables*>(tables);
  if (pcm_is_int16)
    hipLaunchKernelGGL(fbank_kernel<true>, dim3(grid), dim3(64 * FB_WAVES), 0, stream, tab, pcm, (long)ld_pcm, n_samples, B, T,
                       num_mel_bins, feat, (long)ld_feat, feat_len);
  else
    hipLaunchKernelGGL(fbank_kernel<false>, dim3(grid), dim3(64 * FB_WAVES), 0, stream, tab, pcm, (long)ld_pcm, n_samples, B, T,
                       num_mel_bins, feat, (long)ld_feat, feat_len);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
