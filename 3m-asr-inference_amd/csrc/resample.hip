// Audio in at any sample rate: Kaldi's LinearResample on the device: samples at rate_in -> samples at rate_out.
//
// Contract (ResampleWaveform as compute-fbank-feats calls it): a windowed-sinc low-pass at cutoff = 0.99 * 0.5 * min(ri, ro)
// with Z = 6 zero crossings on either side, ww = Z / (2 cutoff).  The filter only depends on the output's phase
// p = o % out_unit (out_unit = ro / gcd): first[p] = ceil((p / ro - ww) ri), n[p] = floor((p / ro + ww) ri) - first[p] + 1,
// w[p][j] = window(dt) filt(dt) / ri at dt = (first[p] + j) / ri - p / ro, and
//     y[o] = sum_j w[p][j] x[first[p] + (o / out_unit) in_unit + j],        x = 0 outside the signal.
// ri == ro is the identity (one phase, one tap of 1.0): the feature pipeline does not resample then.
//
// Layout: a work-group of 256 lanes owns 1024 consecutive outputs of one row, in passes of `sub` <= 1024 outputs whose input
// span fits the 16 KiB LDS stage (sub = 1024 up to 48 kHz -> 16 kHz, 670 at 96 kHz).  A pass stages the span as mono fp32 (int16 -> float and
// the channel mean happen on the way in), then lane l computes outputs l, l + 256, l + 512, l + 768 of the pass, each on its
// own: one fp32 accumulator from 0, its n[p] taps in ascending j, multiply then add (the library is built with
// -ffp-contract=off).  Weights are phase-minor, w[j][p], so the lanes of a wave (consecutive outputs = consecutive phases)
// read consecutive floats.  No atomics, no cross-lane step: an
// output's bits depend on its absolute index, its tap inputs and the table only.  Tables are built on the HOST in float64
// and rounded once; the kernel calls no math library.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "kernels.h"

namespace m3 {

namespace {

constexpr int RS_THREADS = 256, RS_PER_LANE = 4, RS_TILE = RS_THREADS * RS_PER_LANE, RS_LDS = 4096, RS_MAX_TAPS = 512, RS_ZEROS = 6;
constexpr int RS_MIN_RATE = 1000, RS_MAX_RATE = 384000;
constexpr long RS_MAX_FLOATS = 1l << 20;

// The device image: this header, first[out_unit], n[out_unit] (int32, padded to 16 bytes), then w[max_taps][out_unit] floats
// (zero where j >= n[p]).
struct ResampleHeader {
  int32_t rate_in, rate_out, in_unit, out_unit, max_taps;
  int32_t w_offset;                     // of the weights, in 4-byte words from the start of the image
  int32_t reserved[2];
};
static_assert(sizeof(ResampleHeader) == 32, "the table image is read with 16-byte alignment");

struct Rates {
  int ri, ro, in_unit, out_unit;
  bool identity;
  double cutoff, ww;
};

int gcd_of(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

Rates rates_of(int ri, int ro) {
  Rates r;
  const int g = gcd_of(ri, ro);
  r.ri = ri;
  r.ro = ro;
  r.in_unit = ri / g;
  r.out_unit = ro / g;
  r.identity = ri == ro;
  r.cutoff = 0.99 * 0.5 * (double)(ri < ro ? ri : ro);
  r.ww = RS_ZEROS / (2.0 * r.cutoff);
  return r;
}

// first input (relative to (o / out_unit) * in_unit) and tap count of phase p
void phase_span(const Rates& r, int p, long* first, long* n) {
  if (r.identity) {
    *first = 0;
    *n = 1;
    return;
  }
  const double t = (double)p / (double)r.ro;
  *first = (long)ceil((t - r.ww) * (double)r.ri);
  *n = (long)floor((t + r.ww) * (double)r.ri) - *first + 1;
}

double filter_weight(const Rates& r, double dt) {
  const double pi = 3.14159265358979323846;
  const double window = fabs(dt) < r.ww ? 0.5 * (1.0 + cos(2.0 * pi * r.cutoff / RS_ZEROS * dt)) : 0.0;
  const double filt = dt != 0.0 ? sin(2.0 * pi * r.cutoff * dt) / (pi * dt) : 2.0 * r.cutoff;
  return window * filt / (double)r.ri;
}

int rates_ok(int ri, int ro) {
  M3_REQUIRE(ri >= RS_MIN_RATE && ri <= RS_MAX_RATE, "resample: rate_in=%d outside [%d, %d]", ri, RS_MIN_RATE, RS_MAX_RATE);
  M3_REQUIRE(ro >= RS_MIN_RATE && ro <= RS_MAX_RATE, "resample: rate_out=%d outside [%d, %d]", ro, RS_MIN_RATE, RS_MAX_RATE);
  return 0;
}

// max_taps of the pair; refuses what the kernel or the image cannot hold
int table_shape(const Rates& r, int* max_taps) {
  // n[p] <= 2 ww ri + 1 for every phase: refuse before walking up to 384000 phases
  M3_REQUIRE(2.0 * r.ww * (double)r.ri - 1.0 <= (double)RS_MAX_TAPS || r.identity,
             "resample: %d -> %d Hz needs more than %d taps per output (max_taps)", r.ri, r.ro, RS_MAX_TAPS);
  long most = 0;
  for (int p = 0; p < r.out_unit; ++p) {
    long first, n;
    phase_span(r, p, &first, &n);
    most = n > most ? n : most;
  }
  M3_REQUIRE(most <= RS_MAX_TAPS, "resample: %d -> %d Hz needs %ld taps per output (max_taps), more than %d", r.ri, r.ro, most,
             RS_MAX_TAPS);
  M3_REQUIRE(most * (long)r.out_unit <= RS_MAX_FLOATS, "resample: the table of %d -> %d Hz holds %d phases x %ld taps = %ld floats, more than %ld",
             r.ri, r.ro, r.out_unit, most, most * (long)r.out_unit, RS_MAX_FLOATS);
  *max_taps = (int)most;
  return 0;
}

size_t index_words(int out_unit) { return align_up(2 * (size_t)out_unit, 4); }

__device__ __forceinline__ float pcm_at(const void* row, long i, bool int16) {
  return int16 ? (float)reinterpret_cast<const int16_t*>(row)[i] : reinterpret_cast<const float*>(row)[i];
}

template <bool INT16>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const int32_t* __restrict__ tab, const void* __restrict__ pcm, int C,
                                                              int channel, long ld_pcm, const int64_t* __restrict__ in0,
                                                              const int32_t* __restrict__ n_in, const int64_t* __restrict__ out0,
                                                              const int32_t* __restrict__ n_out, int N_out,
                                                              float* __restrict__ out, long ld_out) {
  __shared__ float xs[RS_LDS];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile0 = blockIdx.x * RS_TILE;                        // < N_out
  const int tile_n = min(RS_TILE, N_out - tile0);
  const long o_row = out0[b];
  int want = n_out[b];
  want = o_row < 0 ? 0 : min(max(want, 0), N_out);               // an output before sample 0 of the session does not exist
  float* const orow = out + (long)b * ld_out + tile0;
  const int live = min(max(want - tile0, 0), tile_n);            // outputs of this tile that are computed; the rest are zeros
  for (int i = live + tid; i < tile_n; i += RS_THREADS) orow[i] = 0.f;
  if (live == 0) return;

  // a table that is not one of ours must not become an address
  const int in_unit = max(tab[2], 1), out_unit = max(tab[3], 1), max_taps = min(max(tab[4], 1), RS_MAX_TAPS);
  const int32_t* const t_first = tab + sizeof(ResampleHeader) / 4;
  const int32_t* const t_n = t_first + out_unit;
  const float* const t_w = reinterpret_cast<const float*>(tab + max(tab[5], 0));
  long n_row = n_in[b];
  n_row = min(max(n_row, 0l), ld_pcm / C);                       // a row holds ld_pcm / C samples per channel at most
  const long i_row = in0[b];
  const char* const prow = reinterpret_cast<const char*>(pcm) + (long)b * ld_pcm * (INT16 ? 2 : 4);
  // outputs per pass: (sub - 1) ri / ro + max_taps + 2 input samples must fit the stage
  const int sub = (int)min((long)RS_TILE, max(1l, (long)(RS_LDS - max_taps - 2) * out_unit / in_unit));

  for (int s0 = 0; s0 < live; s0 += sub) {
    const int cnt = min(sub, live - s0);
    const long o0 = o_row + tile0 + s0;                          // absolute index of the pass's first output
    const long u0 = o0 / out_unit;
    const int p0 = (int)(o0 - u0 * out_unit);
    // the input span of the pass: first input of its first output .. last input of its last output (both monotone in o)
    const int q_last = p0 + cnt - 1, du_last = q_last / out_unit, p_last = q_last - du_last * out_unit;
    const long begin = (long)t_first[p0] + u0 * in_unit;
    const long end = (long)t_first[p_last] + (u0 + du_last) * in_unit + min(max(t_n[p_last], 0), max_taps);
    const int len = (int)min(max(end - begin, 0l), (long)RS_LDS);
    const long e_lo = begin - i_row;                             // the span in samples of the row: [e_lo, e_lo + len)
    // each lane's outputs of the pass, tid + 256 k: where their taps start in the stage, and how many (loads that do not
    // wait for the stage)
    int tap0[RS_PER_LANE], taps[RS_PER_LANE], phase[RS_PER_LANE];
#pragma unroll
    for (int k = 0; k < RS_PER_LANE; ++k) {
      const int i = tid + RS_THREADS * k;
      tap0[k] = taps[k] = phase[k] = 0;
      if (i < cnt) {
        const int q = p0 + i, du = q / out_unit, p = q - du * out_unit;
        const long s = (long)t_first[p] + (u0 + du) * in_unit - begin;
        const int n = min(max(t_n[p], 0), max_taps);
        const bool inside = s >= 0 && s + n <= len;              // (always, with a table of ours)
        phase[k] = p;
        tap0[k] = inside ? (int)s : 0;
        taps[k] = inside ? n : 0;
      }
    }
    __syncthreads();                                             // the previous pass has read its stage
    if (C == 1) {
      // mono: whole 16-byte pieces of the row, converted on the way into LDS
      constexpr int E = INT16 ? 8 : 4;
      const long k0 = (e_lo >= 0 ? e_lo : e_lo - (E - 1)) / E;   // floor
      for (long k = k0 + tid; k * E < e_lo + len; k += RS_THREADS) {
        const long base = k * E;
        float v[E];
#pragma unroll
        for (int q = 0; q < E; ++q) v[q] = 0.f;
        if (base >= 0 && base < n_row) {                         // base + E <= ld_pcm: rows are whole 16-byte pieces
          if (INT16) {
            const u32x4 r = ldg16b(prow + base * 2);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              v[2 * q] = (float)(int16_t)(r[q] & 0xffffu);
              v[2 * q + 1] = (float)(int16_t)(r[q] >> 16);
            }
          } else {
            const f32x4 r = ldg4(reinterpret_cast<const float*>(prow) + base);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = r[q];
          }
        }
#pragma unroll
        for (int q = 0; q < E; ++q) {
          const long li = base + q - e_lo;
          if (li >= 0 && li < len) xs[li] = base + q < n_row ? v[q] : 0.f;
        }
      }
    } else {
      for (int i = tid; i < len; i += RS_THREADS) {
        const long s = e_lo + i;
        float v = 0.f;
        if (s >= 0 && s < n_row) {
          if (channel >= 0) {
            v = pcm_at(prow, s * C + channel, INT16);
          } else {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a += pcm_at(prow, s * C + c, INT16);
            v = a / (float)C;
          }
        }
        xs[i] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS_PER_LANE; ++k) {
      const int i = tid + RS_THREADS * k;
      if (i < cnt) {
        const float* const x = xs + tap0[k];
        const float* w = t_w + phase[k];
        float acc = 0.f;
        for (int j = 0; j < taps[k]; ++j, w += out_unit) acc += *w * x[j];
        orow[s0 + i] = acc;
      }
    }
  }
}

}  // namespace

// Outputs available from n_in input samples (Kaldi's GetNumOutputSamples); flush: the stream has ended.
long resample_num_samples(int ri, int ro, long n_in, int flush) {
  const Rates r = rates_of(ri, ro);
  if (n_in <= 0) return 0;
  if (r.identity) return n_in;
  const long tick = (long)r.in_unit * (long)ro;                  // lcm(ri, ro); tick / ri = out_unit, tick / ro = in_unit
  long L = n_in * (long)r.out_unit;
  if (!flush) L -= (long)floor(r.ww * (double)tick);
  if (L <= 0) return 0;
  long last = L / r.in_unit;
  if (last * r.in_unit == L) --last;
  return last + 1;
}

// [first_in, end_in): the absolute input indices that outputs [out0, out0 + n_out) read (empty at the first output's start
// when n_out <= 0)
void resample_input_span(int ri, int ro, long out0, long n_out, long* first_in, long* end_in) {
  const Rates r = rates_of(ri, ro);
  long first, n;
  phase_span(r, (int)(out0 % r.out_unit), &first, &n);
  *first_in = *end_in = first + out0 / r.out_unit * r.in_unit;
  if (n_out <= 0) return;
  const long last = out0 + n_out - 1;
  phase_span(r, (int)(last % r.out_unit), &first, &n);
  *end_in = first + last / r.out_unit * r.in_unit + n;
}

size_t resample_tables_bytes(int ri, int ro) {
  if (rates_ok(ri, ro)) return 0;
  const Rates r = rates_of(ri, ro);
  int max_taps = 0;
  if (table_shape(r, &max_taps)) return 0;
  return sizeof(ResampleHeader) + 4 * (index_words(r.out_unit) + align_up((size_t)max_taps * r.out_unit, 4));
}

// The tables in float64, every weight rounded once to float32, into a host image of resample_tables_bytes() bytes.
int resample_tables_build(int ri, int ro, void* host_image) {
  if (int rc = rates_ok(ri, ro)) return rc;
  const Rates r = rates_of(ri, ro);
  int max_taps = 0;
  if (int rc = table_shape(r, &max_taps)) return rc;
  const size_t bytes = sizeof(ResampleHeader) + 4 * (index_words(r.out_unit) + align_up((size_t)max_taps * r.out_unit, 4));
  memset(host_image, 0, bytes);
  ResampleHeader* h = reinterpret_cast<ResampleHeader*>(host_image);
  h->rate_in = ri;
  h->rate_out = ro;
  h->in_unit = r.in_unit;
  h->out_unit = r.out_unit;
  h->max_taps = max_taps;
  h->w_offset = (int32_t)(sizeof(ResampleHeader) / 4 + index_words(r.out_unit));
  int32_t* const t_first = reinterpret_cast<int32_t*>(h + 1);
  int32_t* const t_n = t_first + r.out_unit;
  float* const w = reinterpret_cast<float*>(host_image) + h->w_offset;
  for (int p = 0; p < r.out_unit; ++p) {
    long first, n;
    phase_span(r, p, &first, &n);
    t_first[p] = (int32_t)first;
    t_n[p] = (int32_t)n;
    if (r.identity) {
      w[p] = 1.f;
      continue;
    }
    const double t = (double)p / (double)ro;
    for (long j = 0; j < n; ++j) w[j * r.out_unit + p] = (float)filter_weight(r, (double)(first + j) / (double)ri - t);
  }
  return 0;
}

int launch_resample(const void* tables, const void* pcm, int pcm_is_int16, int channels, int channel, int ld_pcm,
                    const int64_t* in0, const int32_t* n_in, const int64_t* out0, const int32_t* n_out, int B, int N_out,
                    float* out, int ld_out, hipStream_t stream) {
  if (B == 0 || N_out == 0) return 0;
  const dim3 grid((unsigned)((N_out + RS_TILE - 1) / RS_TILE), (unsigned)B);
  const int32_t* tab = reinterpret_cast<const int32_t*>(tables);
  if (pcm_is_int16)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), 0, stream, tab, pcm, channels, channel, (long)ld_pcm, in0, n_in,
                       out0, n_out, N_out, out, (long)ld_out);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), 0, stream, tab, pcm, channels, channel, (long)ld_pcm, in0, n_in,
                       out0, n_out, N_out, out, (long)ld_out);
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
