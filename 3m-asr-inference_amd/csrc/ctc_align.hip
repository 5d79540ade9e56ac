// CTC forced alignment: the best CTC alignment of a given token sequence to an utterance's frames -- Viterbi over
// the blank-interleaved trellis -- and from it every token's first frame, end frame, peak frame and peak posterior.
//
//   utterance u: T = n_frames[u] frames, tokens y[0..L) = tokens[tok0[u] .. tok0[u + 1]), S = 2 L + 1 states,
//   lab(s) = blank (s even) | y[s >> 1] (s odd).
//
// Two launches.  ctc_align_emit: one wave per (utterance, frame) takes the fp32 logsumexp of the frame's V logits and keeps the
// L + 1 log-probabilities the trellis can ever ask for: emit[u][t][0] = blank, emit[u][t][1 + i] = y[i].  ctc_align_path: one
// work-group per utterance, serial in t and parallel in s; the score vector lives in LDS, double-buffered (one barrier per
// frame), the moves go as one byte per (t, s) to the caller's workspace, and the backtrace and the span / peak extraction
// follow in the same launch.  Plain loads and vector stores only, no atomics: every word has one writer per launch.
//
// The arithmetic of the path stage is exact by contract (tests/ctc_align_ref.py): one float32 add on a float32 maximum per
// (t, s), ties stay > step > skip.  The library is built with -ffp-contract=off, and there is nothing to contract here anyway.
#include <limits.h>
#include <math.h>

#include "../../include/m3asr.h"
#include "common.h"
#include "kernels.h"

namespace m3 {
namespace {

constexpr int CA_MAX_TOKENS = 4000;        // S = 8001 states: two score vectors of 4 S bytes fit the 64 KB of LDS a launch gets unasked
constexpr int CA_MAX_FRAMES = 1 << 20;
constexpr int CA_MAX_N = 1 << 20;
constexpr int CA_ITEMS = 8;                // states per thread once S exceeds a 1024-thread work-group (1024 * 8 >= 8001)
// frames whose emissions are in flight ahead of the frame being reduced: four where a thread owns one state, two where it owns
// CA_ITEMS (at 1024 threads a lane has 128 VGPRs; four frames of eight states spilled 52 of them)
constexpr int CA_AHEAD = 4, CA_AHEAD_ITEMS = 2;

enum { CA_OK = 0, CA_NO_ALIGNMENT = 1, CA_BAD_INPUT = 2 };

inline int ca_states(int max_tokens) { return 2 * max_tokens + 1; }
inline size_t ca_move_stride(int max_tokens) { return align_up((size_t)ca_states(max_tokens), 64); }   // bytes per frame

int check_align_desc(const m3_ctc_align_desc* d) {
  M3_REQUIRE(d != nullptr, "ctc_align: null descriptor");
  M3_REQUIRE(d->n >= 0 && d->n <= CA_MAX_N, "ctc_align: n = %d outside [0, 2^20]", d->n);
  M3_REQUIRE(d->V >= 1, "ctc_align: V = %d", d->V);
  M3_REQUIRE(d->blank >= 0 && d->blank < d->V, "ctc_align: blank = %d outside [0, V = %d)", d->blank, d->V);
  M3_REQUIRE(d->max_frames >= 0 && d->max_frames <= CA_MAX_FRAMES, "ctc_align: max_frames = %d outside [0, 2^20]", d->max_frames);
  M3_REQUIRE(d->max_tokens >= 0 && d->max_tokens <= CA_MAX_TOKENS, "ctc_align: max_tokens = %d outside [0, %d]", d->max_tokens,
             CA_MAX_TOKENS);
  // int32 index arithmetic of the kernels: a frame's move row and emission row inside one utterance, and the (u, t) wave index
  M3_REQUIRE((size_t)d->max_frames * ca_move_stride(d->max_tokens) <= (size_t)INT_MAX,
             "ctc_align: max_frames = %d x max_tokens = %d overflows the int32 move offsets", d->max_frames, d->max_tokens);
  M3_REQUIRE((size_t)d->n * (size_t)d->max_frames <= (size_t)INT_MAX - 4, "ctc_align: n = %d x max_frames = %d overflows int32", d->n,
             d->max_frames);                     // the emit grid rounds the wave count up to a multiple of four
  return 0;
}

// what the utterance may be asked: T and L inside the descriptor (else CA_BAD_INPUT and nothing of it is read)
__device__ __forceinline__ bool ca_sizes_ok(int T, int L, int max_frames, int max_tokens) {
  return T >= 0 && T <= max_frames && L >= 0 && L <= max_tokens;
}

// ---- stage 1: emissions ------------------------------------------------------------------------------------------------------
// One wave per (u, t).  Rows are 4-byte aligned only (V = 1434, any ldl): the lanes walk the row's 16-byte aligned middle four
// floats at a time and its head and tail (at most three floats each) one at a time.
template <typename F>
__device__ __forceinline__ void ca_row_visit(const float* xr, int V, int lane, F f) {
  const int head = min(V, (int)((16u - ((unsigned)(uintptr_t)xr & 15u)) >> 2) & 3);
  const int quads = (V - head) >> 2;
  if (lane < head) f(xr[lane]);
  for (int q = lane; q < quads; q += 64) {
    const f32x4 v = ldg4(xr + head + 4 * q);
    f(v[0]); f(v[1]); f(v[2]); f(v[3]);
  }
  const int tail0 = head + 4 * quads;
  if (tail0 + lane < V) f(xr[tail0 + lane]);       // V - tail0 <= 3
}

__global__ __launch_bounds__(256) void ctc_align_emit_kernel(const float* __restrict__ logits, int ldl, int V, int blank,
                                                             int n, int max_frames, int max_tokens,
                                                             const int32_t* __restrict__ row0, const int32_t* __restrict__ n_frames,
                                                             const int32_t* __restrict__ tokens, const int32_t* __restrict__ tok0,
                                                             float* __restrict__ emit) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);          // < n * max_frames + 3 <= INT_MAX (checked by the launcher)
  const int u = w / max_frames, t = w - u * max_frames;
  if (u >= n) return;
  const int T = n_frames[u], y0 = tok0[u], L = tok0[u + 1] - y0;
  if (!ca_sizes_ok(T, L, max_frames, max_tokens) || t >= T) return;
  const float* xr = logits + ((size_t)row0[u] + (size_t)t) * (size_t)ldl;
  float mx = -INFINITY;
  ca_row_visit(xr, V, lane, [&](float v) { mx = fmaxf(mx, v); });
  mx = wave_max(mx);
  float sum = 0.f;
  ca_row_visit(xr, V, lane, [&](float v) { sum += expf(v - mx); });
  const float lse = mx + logf(wave_sum(sum));
  float* er = emit + ((size_t)u * max_frames + t) * (size_t)(max_tokens + 1);
  if (lane == 0) er[0] = xr[blank] - lse;
  for (int i = lane; i < L; i += 64) {
    const int y = tokens[y0 + i];
    er[1 + i] = (y >= 0 && y < V) ? xr[y] - lse : -INFINITY;   // a bad token makes the utterance CA_BAD_INPUT in stage 2
  }
}

// ---- stage 2: trellis, backtrace, spans ---------------------------------------------------------------------------------------
// Thread tid owns the states s = tid + j * blockDim.x, j < NI.  Its emission column never changes (0 for a blank state,
// 1 + (s >> 1) for a token state), so the loads of frames t + 1 .. t + AHEAD are issued before frame t is reduced and hang
// off nothing in the dependent chain  LDS read -> max -> add -> LDS write -> barrier.
template <int NI, int AHEAD>
__global__ __launch_bounds__(1024) void ctc_align_path_kernel(int blank, int V, int max_frames, int max_tokens,
                                                              const float* __restrict__ emit, const int32_t* __restrict__ n_frames,
                                                              const int32_t* __restrict__ tokens, const int32_t* __restrict__ tok0,
                                                              unsigned char* __restrict__ moves_all, size_t move_stride,
                                                              float* __restrict__ score, int32_t* __restrict__ status,
                                                              int32_t* __restrict__ state, int32_t* __restrict__ tok_start,
                                                              int32_t* __restrict__ tok_end, int32_t* __restrict__ tok_peak,
                                                              float* __restrict__ tok_logp) {
  extern __shared__ float ca_lds[];                  // two score vectors of S floats
  __shared__ int bad_token;
  const int u = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int T = n_frames[u], y0 = tok0[u], L = tok0[u + 1] - y0;
  int32_t* st_row = state + (size_t)u * max_frames;
  const bool sizes_ok = ca_sizes_ok(T, L, max_frames, max_tokens);

  if (tid == 0) bad_token = 0;
  __syncthreads();
  if (sizes_ok) {
    int bad = 0;
    for (int i = tid; i < L; i += nt) {
      const int y = tokens[y0 + i];
      bad |= (y < 0 || y >= V || y == blank);
    }
    if (bad) bad_token = 1;                          // every writer stores the same value
  }
  __syncthreads();
  int code = (!sizes_ok || bad_token) ? CA_BAD_INPUT : ((T == 0 && L > 0) ? CA_NO_ALIGNMENT : CA_OK);

  const int S = 2 * L + 1;
  const int E = max_tokens + 1;
  const float* er = emit + (size_t)u * max_frames * E;
  unsigned char* moves = moves_all + (size_t)u * max_frames * move_stride;
  float best_score = 0.f;                            // T == 0, L == 0: the empty alignment
  int final_state = 0;

  if (code == CA_OK && T > 0) {
    float* a_cur = ca_lds;
    float* a_nxt = ca_lds + S;
    int col[NI];                                     // emission column of each owned state, -1: not a state
    bool skip_ok[NI];
    float ahead[NI][AHEAD];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int s = tid + j * nt;
      col[j] = s < S ? ((s & 1) ? 1 + (s >> 1) : 0) : -1;
      skip_ok[j] = s < S && (s & 1) && s >= 3 && tokens[y0 + (s >> 1)] != tokens[y0 + (s >> 1) - 1];
      if (col[j] >= 0) {
        a_cur[s] = s < 2 ? er[col[j]] : -INFINITY;   // frame 0
        moves[s] = 0;
      }
#pragma unroll
      for (int k = 0; k < AHEAD; ++k) ahead[j][k] = (col[j] >= 0 && 1 + k < T) ? er[(size_t)(1 + k) * E + col[j]] : 0.f;
    }
    __syncthreads();
    for (int t0 = 1; t0 < T; t0 += AHEAD) {
#pragma unroll
      for (int k = 0; k < AHEAD; ++k) {
        const int t = t0 + k;
        if (t < T) {                                 // uniform over the work-group
#pragma unroll
          for (int j = 0; j < NI; ++j) {
            if (col[j] >= 0) {
              const int s = tid + j * nt;
              const float e = ahead[j][k];
              if (t + AHEAD < T) ahead[j][k] = er[(size_t)(t + AHEAD) * E + col[j]];
              float best = a_cur[s];
              int mv = 0;
              const float step = s >= 1 ? a_cur[s - 1] : -INFINITY;
              if (step > best) { best = step; mv = 1; }
              const float skip = skip_ok[j] ? a_cur[s - 2] : -INFINITY;
              if (skip > best) { best = skip; mv = 2; }
              a_nxt[s] = best + e;
              moves[(size_t)t * move_stride + s] = (unsigned char)mv;
            }
          }
          __syncthreads();
          float* tmp = a_cur; a_cur = a_nxt; a_nxt = tmp;
        }
      }
    }
    final_state = S - 1;
    if (S > 1 && a_cur[S - 2] > a_cur[S - 1]) final_state = S - 2;
    best_score = a_cur[final_state];
    if (best_score == -INFINITY) code = CA_NO_ALIGNMENT;
  }

  // backtrace: T dependent one-byte loads by one thread (the moves were stored by this work-group, before the barriers above)
  if (code == CA_OK && tid == 0) {
    int s = final_state;
    for (int t = T - 1; t >= 1; --t) {
      st_row[t] = s;
      s = max(s - (int)moves[(size_t)t * move_stride + s], 0);
    }
    if (T > 0) st_row[0] = s;
  }
  __syncthreads();

  if (tid == 0) {
    score[u] = code == CA_OK ? best_score : -INFINITY;
    status[u] = code;
  }
  const int T_ok = code == CA_OK ? T : 0;
  for (int t = T_ok + tid; t < max_frames; t += nt) st_row[t] = -1;
  if (L <= 0) return;                                // also a corrupt tok0: no per-token output is derived from it
  int32_t* ts = tok_start + y0;
  int32_t* te = tok_end + y0;
  if (code != CA_OK) {
    for (int i = tid; i < L; i += nt) {
      ts[i] = te[i] = tok_peak[y0 + i] = -1;
      tok_logp[y0 + i] = -INFINITY;
    }
    return;
  }
  // a token's frames are one run of the path: its first frame is where the run begins, its end where the run stops
  for (int t = tid; t < T; t += nt) {
    const int s = st_row[t];
    if (s & 1) {
      if (t == 0 || st_row[t - 1] != s) ts[s >> 1] = t;
      if (t == T - 1 || st_row[t + 1] != s) te[s >> 1] = t + 1;
    }
  }
  __syncthreads();
  for (int i = tid; i < L; i += nt) {
    const int b = min(max(ts[i], 0), T), e = min(max(te[i], b), T);
    float pk = -INFINITY;
    int at = b;
    for (int t = b; t < e; ++t) {
      const float v = er[(size_t)t * E + 1 + i];
      if (t == b || v > pk) { pk = v; at = t; }
    }
    tok_peak[y0 + i] = at;
    tok_logp[y0 + i] = pk;
  }
}

}  // namespace

size_t ctc_align_workspace_size(const m3_ctc_align_desc* d) {
  if (check_align_desc(d)) return 0;
  const size_t bytes = (size_t)d->n * (size_t)d->max_frames * ca_move_stride(d->max_tokens);
  return align_up(bytes > 0 ? bytes : 1, 256);       // never 0 for a descriptor the library takes
}

int launch_ctc_align_emit(const m3_ctc_align_desc* d, const float* logits, int ldl, const int32_t* row0, const int32_t* n_frames,
                          const int32_t* tokens, const int32_t* tok0, float* emit, hipStream_t stream) {
  if (int rc = check_align_desc(d)) return rc;
  M3_REQUIRE(ldl >= d->V, "ctc_align_emit: ldl = %d < V = %d", ldl, d->V);
  if (d->n == 0 || d->max_frames == 0) return 0;
  M3_REQUIRE(logits != nullptr && row0 != nullptr && n_frames != nullptr && tok0 != nullptr && emit != nullptr,
             "ctc_align_emit: null pointer");
  M3_REQUIRE(d->max_tokens == 0 || tokens != nullptr, "ctc_align_emit: null token list");
  M3_REQUIRE(((uintptr_t)logits & 3) == 0, "ctc_align_emit: logits must be 4-byte aligned");
  const int waves = d->n * d->max_frames;
  hipLaunchKernelGGL(ctc_align_emit_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, stream, logits, ldl, d->V, d->blank, d->n,
                     d->max_frames, d->max_tokens, row0, n_frames, tokens, tok0, emit);
  M3_LAUNCH_CHECK();
  return 0;
}

int launch_ctc_align_path(const m3_ctc_align_desc* d, const float* emit, const int32_t* n_frames, const int32_t* tokens,
                          const int32_t* tok0, void* workspace, size_t ws_bytes, float* score, int32_t* status, int32_t* state,
                          int32_t* tok_start, int32_t* tok_end, int32_t* tok_peak, float* tok_logp, hipStream_t stream) {
  if (int rc = check_align_desc(d)) return rc;
  const size_t need = ctc_align_workspace_size(d);
  M3_REQUIRE(ws_bytes >= need, "ctc_align_path: workspace %zu bytes < required %zu", ws_bytes, need);
  if (d->n == 0) return 0;
  M3_REQUIRE(workspace != nullptr && n_frames != nullptr && tok0 != nullptr && score != nullptr && status != nullptr,
             "ctc_align_path: null pointer");
  M3_REQUIRE(d->max_frames == 0 || (emit != nullptr && state != nullptr), "ctc_align_path: null emit / state");
  M3_REQUIRE(d->max_tokens == 0 || (tokens != nullptr && tok_start != nullptr && tok_end != nullptr && tok_peak != nullptr &&
                                    tok_logp != nullptr), "ctc_align_path: null token pointer");
  const int S = ca_states(d->max_tokens);
  const size_t lds = 2 * (size_t)S * sizeof(float);
  if (S <= 1024) {
    hipLaunchKernelGGL((ctc_align_path_kernel<1, CA_AHEAD>), dim3((unsigned)d->n), dim3((unsigned)(cdiv(S, 64) * 64)), lds, stream, d->blank, d->V,
                       d->max_frames, d->max_tokens, emit, n_frames, tokens, tok0, (unsigned char*)workspace,
                       ca_move_stride(d->max_tokens), score, status, state, tok_start, tok_end, tok_peak, tok_logp);
  } else {
    hipLaunchKernelGGL((ctc_align_path_kernel<CA_ITEMS, CA_AHEAD_ITEMS>), dim3((unsigned)d->n), dim3(1024), lds, stream, d->blank, d->V, d->max_frames,
                       d->max_tokens, emit, n_frames, tokens, tok0, (unsigned char*)workspace, ca_move_stride(d->max_tokens), score,
                       status, state, tok_start, tok_end, tok_peak, tok_logp);
  }
  M3_LAUNCH_CHECK();
  return 0;
}

}  // namespace m3
