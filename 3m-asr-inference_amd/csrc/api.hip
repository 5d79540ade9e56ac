// C-ABI entry points of libm3asr_hip.so that are thin wrappers over the kernel launchers
// (include/m3asr.h documents which reference interface each one replaces).
#include <string.h>

#include <vector>

#include "../../include/m3asr.h"
#include "common.h"
#include "kernels.h"

namespace m3 {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

// workspace layout of the fused FMoE op (all sections 256-B aligned, as kAlignment in
// the reference's common/common.h:43)
struct MoeWorkspace {
  int32_t* mapping;
  int32_t* acc;
  int32_t* pos;
  float* slab;
  size_t bytes;
};
MoeWorkspace carve_moe_workspace(void* base, int S, int E, int D, int F) {
  MoeWorkspace w;
  size_t off = 0;
  char* p = (char*)base;
  w.mapping = (int32_t*)(p + off); off += align_up((size_t)S * 4, 256);
  w.acc = (int32_t*)(p + off);     off += align_up((size_t)(E + 1) * 4, 256);
  w.pos = (int32_t*)(p + off);     off += align_up((size_t)S * 4, 256);
  w.slab = (float*)(p + off);      off += align_up(expert_ffn_slab_bytes(S, D, F), 256);
  w.bytes = off;
  return w;
}

int moe_expert_ffn_dt(const float* x, const int32_t* gate_idx, const float* w1, const float* b1, const float* w2,
                      const float* b2, int S, int E, int D, int F, const float* gate_value, const float* resid,
                      float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* ws,
                      size_t ws_bytes, hipStream_t stream, ExpertWeights weights, const float* s1 = nullptr, const float* s2 = nullptr, float h_scale = 0.f, const void* xq = nullptr,
                      const float* xq_scale = nullptr, int ldx = 0, int w_layout = EXPERT_W_REF) {
  M3_REQUIRE(S >= 0 && E > 0 && D > 0 && F > 0, "fmoe_expert: bad sizes S=%d E=%d D=%d F=%d", S, E, D, F);
  if (S == 0) return 0;
  MoeWorkspace w = carve_moe_workspace(ws, S, E, D, F);
  M3_REQUIRE(ws != nullptr && ws_bytes >= w.bytes, "fmoe_expert: workspace %zu bytes < required %zu", ws_bytes,
             w.bytes);
  int rc = launch_moe_index(gate_idx, S, E, w.mapping, w.acc, w.pos, stream);
  if (rc) return rc;
  const ExpertFfnPlan plan = plan_expert_ffn(weights, S, E, D, F);
  ExpertFfnArgs a{};
  a.x = x; a.ldx = ldx > 0 ? ldx : D; a.pos = w.pos; a.acc_hist = w.acc; a.w1 = w1; a.w2 = w2; a.s1 = s1; a.s2 = s2; a.b1 = b1;
  a.h_scale = h_scale; a.slab = w.slab; a.xq = xq; a.xq_scale = xq_scale; a.w2_sliced = w_layout;
  rc = launch_expert_ffn(plan, S, E, D, F, a, stream);
  if (rc) return rc;
  return launch_moe_combine(plan.rows(w.slab), plan.slices, w.mapping, gate_idx, gate_value, b2, resid, alpha, ln_gamma, ln_beta, ln_eps,
                            y, S, D, stream);
}

int moe_expert_ffn(const float* x, const int32_t* gate_idx, const float* w1, const float* b1, const float* w2,
                   const float* b2, int S, int E, int D, int F, const float* gate_value, const float* resid,
                   float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* ws,
                   size_t ws_bytes, hipStream_t stream) {
  return moe_expert_ffn_dt(x, gate_idx, w1, b1, w2, b2, S, E, D, F, gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps,
                           y, ws, ws_bytes, stream, ExpertWeights::F32);
}

}  // namespace m3

using namespace m3;

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // (NULL counts as aligned)

// The prefix beam search's entry points say which form they are, fill a BeamCall (kernels.h) and call.
static BeamCall beam_call(const char* who, BeamForm form, const m3_ctc_beam_desc* d, const void* state, size_t bytes, m3_stream stream) {
  BeamCall c{};
  c.who = who; c.form = form; c.d = d; c.state = const_cast<void*>(state); c.bytes = bytes; c.stream = (hipStream_t)stream;
  return c;
}
// *_reset_slots on a *_reset record: an empty list is no work, whatever else stands in the call
static int beam_reset_slots(BeamCall c, const int32_t* slots, int n) {
  M3_REQUIRE(n == 0 || slots != nullptr, "%s_slots: null slot list", c.who);
  if (n == 0) return 0;
  c.slots = slots; c.n = n;
  return beam_reset(c);
}

extern "C" {

int m3_abi_version(void) { return M3ASR_ABI_VERSION; }
const char* m3_last_error(void) { return m3::last_error(); }

int m3_moe_scatter_mapping(const int32_t* gate_idx, int S, int num_expert, int32_t* mapping, int32_t* acc_histogram,
                           int32_t* pos, m3_stream stream) {
  M3_REQUIRE(gate_idx && mapping && acc_histogram, "moe_scatter_mapping: null pointer");
  return launch_moe_index(gate_idx, S, num_expert, mapping, acc_histogram, pos, (hipStream_t)stream);
}
int m3_moe_local_scatter(const void* x, const int32_t* mapping, int S, int row_bytes, void* out, m3_stream stream) {
  return launch_local_scatter(x, mapping, S, row_bytes, out, (hipStream_t)stream);
}
int m3_moe_local_gather(const void* buf, const int32_t* mapping, int S, int row_bytes, void* out, m3_stream stream) {
  return launch_local_gather(buf, mapping, S, row_bytes, out, (hipStream_t)stream);
}
int m3_moe_expert_slice(void) { return kExpertSlice; }
size_t m3_moe_expert_workspace_size(int S, int num_expert, int idim, int hidden_units) {
  if (S <= 0 || hidden_units % kExpertSlice) return 0;
  return carve_moe_workspace(nullptr, S, num_expert, idim, hidden_units).bytes;
}
int m3_moe_expert_ffn(const float* x, const int32_t* gate_idx, const float* w1, const float* b1, const float* w2,
                      const float* b2, int S, int num_expert, int idim, int hidden_units, const float* gate_value,
                      const float* resid, float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps,
                      float* y, void* workspace, size_t workspace_bytes, m3_stream stream) {
  return moe_expert_ffn(x, gate_idx, w1, b1, w2, b2, S, num_expert, idim, hidden_units, gate_value, resid, alpha,
                        ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes, (hipStream_t)stream);
}
// w1 / w2 in fragment order (launch_expert_ffn takes them on the fp32 slab form alone and refuses the rest)
int m3_moe_expert_ffn_wfrag(const float* x, const int32_t* gate_idx, const float* w1, const float* b1, const float* w2,
                            const float* b2, int S, int num_expert, int idim, int hidden_units, const float* gate_value,
                            const float* resid, float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps,
                            float* y, void* workspace, size_t workspace_bytes, m3_stream stream) {
  return moe_expert_ffn_dt(x, gate_idx, w1, b1, w2, b2, S, num_expert, idim, hidden_units, gate_value, resid, alpha, ln_gamma, ln_beta,
                           ln_eps, y, workspace, workspace_bytes, (hipStream_t)stream, ExpertWeights::F32, nullptr, nullptr, 0.f, nullptr,
                           nullptr, 0, EXPERT_W_FRAG);
}
int m3_moe_expert_ffn_bf16(const float* x, const int32_t* gate_idx, const void* w1, const float* b1, const void* w2,
                           const float* b2, int S, int num_expert, int idim, int hidden_units, const float* gate_value,
                           const float* resid, float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps,
                           float* y, void* workspace, size_t workspace_bytes, m3_stream stream) {
  return moe_expert_ffn_dt(x, gate_idx, (const float*)w1, b1, (const float*)w2, b2, S, num_expert, idim, hidden_units,
                           gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes,
                           (hipStream_t)stream, ExpertWeights::BF16);
}
int m3_moe_expert_ffn_fp8(const float* x, const int32_t* gate_idx, const void* w1, const float* w1_scale, const float* b1,
                          const void* w2, const float* w2_scale, const float* b2, int S, int num_expert, int idim,
                          int hidden_units, const float* gate_value, const float* resid, float alpha,
                          const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                          size_t workspace_bytes, m3_stream stream) {
  M3_REQUIRE(w1_scale && w2_scale, "fmoe_expert fp8: null scale");
  return moe_expert_ffn_dt(x, gate_idx, (const float*)w1, b1, (const float*)w2, b2, S, num_expert, idim, hidden_units,
                           gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes,
                           (hipStream_t)stream, ExpertWeights::FP8, w1_scale, w2_scale);
}
int m3_moe_expert_ffn_mxfp4_ldx(const float* x, int ldx, const int32_t* gate_idx, const void* w1, const void* w1_scale, const float* b1,
                                const void* w2, const void* w2_scale, const float* b2, int S, int num_expert, int idim,
                                int hidden_units, const float* gate_value, const float* resid, float alpha,
                                const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                                size_t workspace_bytes, m3_stream stream) {
  M3_REQUIRE(x && gate_idx && w1 && w2 && b1 && y, "fmoe_expert mxfp4: null pointer");
  M3_REQUIRE(w1_scale && w2_scale, "fmoe_expert mxfp4: null scale");
  M3_REQUIRE(idim > 0 && idim % 128 == 0 && hidden_units > 0 && hidden_units % 64 == 0,
             "fmoe_expert mxfp4: idim=%d must be a multiple of 128 and hidden_units=%d of 64", idim, hidden_units);
  M3_REQUIRE(ldx >= idim && (ldx & 3) == 0, "fmoe_expert mxfp4: ldx=%d must be a multiple of 4 and at least idim=%d", ldx, idim);
  M3_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2), "fmoe_expert mxfp4: x / w1 / w2 must be 16-byte aligned");
  return moe_expert_ffn_dt(x, gate_idx, (const float*)w1, b1, (const float*)w2, b2, S, num_expert, idim, hidden_units,
                           gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes,
                           (hipStream_t)stream, ExpertWeights::MXFP4, (const float*)w1_scale, (const float*)w2_scale, 0.f, nullptr,
                           nullptr, ldx);
}
int m3_moe_expert_ffn_mxfp4(const float* x, const int32_t* gate_idx, const void* w1, const void* w1_scale, const float* b1,
                            const void* w2, const void* w2_scale, const float* b2, int S, int num_expert, int idim,
                            int hidden_units, const float* gate_value, const float* resid, float alpha,
                            const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                            size_t workspace_bytes, m3_stream stream) {
  return m3_moe_expert_ffn_mxfp4_ldx(x, idim, gate_idx, w1, w1_scale, b1, w2, w2_scale, b2, S, num_expert, idim, hidden_units,
                                     gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes, stream);
}
int m3_moe_expert_ffn_fp8a8(const float* x, const int32_t* gate_idx, const void* w1, const float* w1_scale, const float* b1,
                            const void* w2, const float* w2_scale, const float* b2, float h_scale, int S, int num_expert, int idim,
                            int hidden_units, const float* gate_value, const float* resid, float alpha,
                            const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                            size_t workspace_bytes, m3_stream stream) {
  M3_REQUIRE(w1_scale && w2_scale, "fmoe_expert fp8a8: null scale");
  M3_REQUIRE(h_scale > 0.f, "fmoe_expert fp8a8: h_scale must be positive");
  return moe_expert_ffn_dt(x, gate_idx, (const float*)w1, b1, (const float*)w2, b2, S, num_expert, idim, hidden_units,
                           gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes,
                           (hipStream_t)stream, ExpertWeights::FP8A8, w1_scale, w2_scale, h_scale);
}
int m3_moe_expert_ffn_fp8a8_xq(const float* x, const void* xq, const float* xq_scale, const int32_t* gate_idx, const void* w1,
                               const float* w1_scale, const float* b1, const void* w2, const float* w2_scale, const float* b2,
                               float h_scale, int S, int num_expert, int idim, int hidden_units, const float* gate_value,
                               const float* resid, float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps,
                               float* y, void* workspace, size_t workspace_bytes, m3_stream stream) {
  M3_REQUIRE(w1_scale && w2_scale, "fmoe_expert fp8a8_xq: null scale");
  M3_REQUIRE(h_scale > 0.f, "fmoe_expert fp8a8_xq: h_scale must be positive");
  M3_REQUIRE(xq && xq_scale, "fmoe_expert fp8a8_xq: null quantised rows / scales");
  M3_REQUIRE(m3_moe_expert_ffn_fp8a8_active(S, num_expert, idim, hidden_units) || x != nullptr,
             "fmoe_expert fp8a8_xq: this shape takes the weight-only form, which needs the fp32 rows (x)");
  return moe_expert_ffn_dt(x, gate_idx, (const float*)w1, b1, (const float*)w2, b2, S, num_expert, idim, hidden_units,
                           gate_value, resid, alpha, ln_gamma, ln_beta, ln_eps, y, workspace, workspace_bytes,
                           (hipStream_t)stream, ExpertWeights::FP8A8, w1_scale, w2_scale, h_scale, xq, xq_scale);
}
int m3_quantize_rows_e4m3(const float* x, int ldx, int S, int idim, void* xq, float* scale, m3_stream stream) {
  M3_REQUIRE(S <= 1 || ldx >= idim, "quantize_rows_e4m3: ldx=%d is shorter than a row of %d", ldx, idim);
  M3_REQUIRE(aligned16(x) && aligned16(xq), "quantize_rows_e4m3: x / xq must be 16-byte aligned");
  return launch_quantize_rows_e4m3(x, ldx, S, idim, xq, scale, (hipStream_t)stream);
}
int m3_moe_expert_ffn_fp8a8_active(int S, int num_expert, int idim, int hidden_units) {
  return plan_expert_ffn(ExpertWeights::FP8A8, S, num_expert, idim, hidden_units).kernel == ExpertKernel::FusedFp8 ? 1 : 0;
}
const char* m3_moe_expert_ffn_kernel(int weight_dtype, int fp8_activations, int S, int num_expert, int idim, int hidden_units,
                                     int32_t* launches, int32_t* slices) {
  ExpertWeights w;
  if (weight_dtype == M3_F32 && !fp8_activations) w = ExpertWeights::F32;
  else if (weight_dtype == M3_BF16 && !fp8_activations) w = ExpertWeights::BF16;
  else if (weight_dtype == M3_FP8) w = fp8_activations ? ExpertWeights::FP8A8 : ExpertWeights::FP8;
  else if (weight_dtype == M3_MXFP4 && !fp8_activations) w = ExpertWeights::MXFP4;
  else return nullptr;
  const ExpertFfnPlan plan = plan_expert_ffn(w, S, num_expert, idim, hidden_units);
  if (plan.launches == 0) return nullptr;
  if (launches) *launches = plan.launches;
  if (slices) *slices = plan.slices;
  return plan.label;
}
int m3_moe_combine(const float* rows, const int32_t* mapping, const float* gate_value, const float* resid, float alpha,
                   const float* ln_gamma, const float* ln_beta, float ln_eps, float* out, int S, int idim,
                   m3_stream stream) {
  M3_REQUIRE(rows && mapping && out, "moe_combine: null pointer");
  return launch_moe_combine(rows, 1, mapping, nullptr, gate_value, nullptr, resid, alpha, ln_gamma, ln_beta, ln_eps, out,
                            S, idim, (hipStream_t)stream);
}
int m3_moe_combine_bf16(const float* rows, const int32_t* mapping, const float* gate_value, const float* resid, float alpha,
                        const float* ln_gamma, const float* ln_beta, float ln_eps, float* out, void* out_bf16, int S, int idim,
                        m3_stream stream) {
  M3_REQUIRE(rows && mapping && out, "moe_combine_bf16: null pointer");
  return launch_moe_combine(rows, 1, mapping, nullptr, gate_value, nullptr, resid, alpha, ln_gamma, ln_beta, ln_eps, out,
                            S, idim, (hipStream_t)stream, out_bf16);
}
int m3_ep_send_map(const int32_t* gate_idx, const int32_t* mapping, const int32_t* acc_histogram, int S, int world, int e_loc,
                   int capacity, int32_t* map_send, void* wire, int row_bytes, m3_stream stream) {
  M3_REQUIRE(gate_idx && mapping && acc_histogram && map_send && wire, "ep_send_map: null pointer");
  return launch_ep_send_map(gate_idx, mapping, acc_histogram, S, world, e_loc, capacity, map_send, wire, row_bytes,
                            (hipStream_t)stream);
}
int m3_ep_recv_gate(const void* wire, int world, int e_loc, int capacity, int row_bytes, int32_t* gate_recv, m3_stream stream) {
  M3_REQUIRE(wire && gate_recv, "ep_recv_gate: null pointer");
  return launch_ep_recv_gate(wire, world, e_loc, capacity, row_bytes, gate_recv, (hipStream_t)stream);
}
int m3_moe_router(const float* embed, int ld_embed, int embed_dim, const float* x, int ldx, int idim, const float* w,
                  const float* bias, const float* ln_gamma, const float* ln_beta, float ln_eps, float* xn, int ld_xn,
                  float* logits, int ld_logits, int S, int num_expert, m3_stream stream) {
  // row strides (include/m3asr.h): rows may not overlap; the 16-byte accesses of embed / x / xn need multiples of 4 (launcher)
  M3_REQUIRE(S <= 1 || (ld_embed >= embed_dim && ldx >= idim), "moe_router: ld_embed=%d / ldx=%d shorter than the rows (%d / %d)",
             ld_embed, ldx, embed_dim, idim);
  M3_REQUIRE(S <= 1 || xn == nullptr || ld_xn >= idim, "moe_router: ld_xn=%d is shorter than a row of %d", ld_xn, idim);
  M3_REQUIRE(S <= 1 || ld_logits >= num_expert, "moe_router: ld_logits=%d is shorter than a row of %d", ld_logits, num_expert);
  M3_REQUIRE(aligned16(embed) && aligned16(x) && aligned16(xn), "moe_router: embed / x / xn must be 16-byte aligned");
  return launch_moe_router(embed, ld_embed, embed_dim, x, ldx, idim, w, bias, ln_gamma, ln_beta, ln_eps, xn, ld_xn, logits,
                           ld_logits, S, num_expert, nullptr, (hipStream_t)stream);
}
int m3_softmax_top1(const float* logits, int ld, const int32_t* len, int rows_per_batch, int S, int width,
                    int32_t* idx, float* value, m3_stream stream) {
  M3_REQUIRE(S <= 1 || ld >= width, "softmax_topk: ld=%d is shorter than a row of %d", ld, width);
  return launch_softmax_top1(logits, ld, len, rows_per_batch, S, width, idx, value, (hipStream_t)stream);
}
int m3_moe_gate_index(const float* logits, const int32_t* row_len, int rows_per_batch, int S, int num_expert, int32_t* gate_idx,
                      float* gate_value, int32_t* mapping, int32_t* acc_histogram, int32_t* pos, m3_stream stream) {
  M3_REQUIRE(logits && gate_idx && gate_value && mapping && acc_histogram, "moe_gate_index: null pointer");
  M3_REQUIRE(aligned16(logits), "moe_gate_index: logits must be 16-byte aligned");
  return launch_moe_gate_index(logits, num_expert, row_len, rows_per_batch, S, gate_idx, gate_value, mapping, acc_histogram, pos,
                               (hipStream_t)stream);
}
int m3_moe_route(const float* x, int ldx, int idim, const float* wx, const float* wsum, const float* bias, const float* eall,
                 int ld_e, float ln_eps, const int32_t* row_len, int rows_per_batch, int S, int num_expert, int32_t* gate_idx,
                 float* gate_value, int32_t* mapping, int32_t* acc_histogram, int32_t* pos, m3_stream stream) {
  M3_REQUIRE(x && wx && wsum && gate_idx && gate_value && mapping && acc_histogram, "moe_route: null pointer");
  M3_REQUIRE(idim > 0, "moe_route: idim=%d", idim);
  M3_REQUIRE(S <= 1 || ldx >= idim, "moe_route: ldx=%d is shorter than a row of %d", ldx, idim);
  M3_REQUIRE(eall == nullptr || S <= 1 || ld_e >= num_expert, "moe_route: ld_e=%d is shorter than a row of %d", ld_e, num_expert);
  M3_REQUIRE(aligned16(x) && aligned16(wx), "moe_route: x / wx must be 16-byte aligned");
  return launch_moe_route(x, ldx, idim, wx, wsum, bias, eall, ld_e, ln_eps, row_len, rows_per_batch, S, num_expert, gate_idx,
                          gate_value, mapping, acc_histogram, pos, (hipStream_t)stream);
}
size_t m3_moe_route_expert_workspace_size(int S, int num_expert, int idim, int hidden_units) {
  if (!expert_ffn_f32_self_routing(S, num_expert) || idim <= 0 || hidden_units <= 0 || hidden_units % kExpertSlice) return 0;
  return align_up(expert_ffn_slab_bytes(S, idim, hidden_units), 256);
}
int m3_moe_route_expert_ffn(const float* x, int ldx, const float* logits, const int32_t* row_len, int rows_per_batch,
                            const float* w1, const float* b1, const float* w2, int w2_sliced, const float* b2, int S,
                            int num_expert, int idim, int hidden_units, const float* norm_gamma, const float* norm_beta,
                            float norm_eps, int use_gate_value, const float* resid, float alpha, const float* ln_gamma,
                            const float* ln_beta, float ln_eps, int32_t* gate_idx, float* gate_value, int32_t* mapping,
                            int32_t* acc_histogram, int32_t* pos, float* y, void* workspace, size_t workspace_bytes,
                            m3_stream stream) {
  M3_REQUIRE(x && w1 && b1 && w2 && y, "moe_route_expert_ffn: null pointer");
  M3_REQUIRE((norm_gamma == nullptr) == (norm_beta == nullptr) && (ln_gamma == nullptr) == (ln_beta == nullptr),
             "moe_route_expert_ffn: a LayerNorm needs both gamma and beta");
  M3_REQUIRE(idim > 0 && hidden_units > 0, "moe_route_expert_ffn: bad sizes D=%d F=%d", idim, hidden_units);
  M3_REQUIRE(S <= 1 || ldx >= idim, "moe_route_expert_ffn: ldx=%d is shorter than a row of %d", ldx, idim);
  M3_REQUIRE(aligned16(x) && aligned16(logits), "moe_route_expert_ffn: x / logits must be 16-byte aligned");
  const size_t need = m3_moe_route_expert_workspace_size(S, num_expert, idim, hidden_units);
  M3_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), "moe_route_expert_ffn: workspace %zu bytes < required %zu",
             workspace_bytes, need);      // (need == 0: a shape the launcher rejects, with its own message)
  float* slab = (float*)workspace;
  int rc = launch_expert_route_ffn_f32(x, ldx, logits, row_len, rows_per_batch, S, num_expert, idim, hidden_units, w1, b1, w2, w2_sliced,
                                       b2, slab, gate_idx, gate_value, mapping, acc_histogram, pos, (hipStream_t)stream, norm_gamma,
                                       norm_beta, norm_eps);
  if (rc) return rc;
  return launch_moe_combine(slab, hidden_units / kExpertSlice, nullptr, gate_idx, use_gate_value ? gate_value : nullptr, nullptr, resid,
                            alpha, ln_gamma, ln_beta, ln_eps, y, S, idim, (hipStream_t)stream);
}

// The attention core at the boundary: the record from the ABI descriptor plus what only the boundary asks of the row operands
// besides the multiples the launcher checks (include/m3asr.h).  pair < 0: a single entry; 0 / 1: a problem of m3_relpos_attention_pair.
static int attention_args_from_desc(const m3_attention_desc* d, const char* who, int pair, AttArgs* q) {
  if (pair >= 0) M3_REQUIRE(d->B > 0 && d->T > 0 && d->H > 0 && d->dk > 0, "%s: empty problem %d", who, pair);
  M3_REQUIRE((pair < 0 && (d->B <= 0 || d->T <= 0 || d->H <= 0)) || (d->qkv && d->p && d->pos_u && d->pos_v && d->out),
             "%s: null qkv / p / pos_u / pos_v / out", who);
  M3_REQUIRE(d->B * d->T <= 1 || (d->ldq >= 3 * d->H * d->dk && d->ldo >= d->H * d->dk), "attention: ldq=%d / ldo=%d shorter than the rows (%d / %d)",
             d->ldq, d->ldo, 3 * d->H * d->dk, d->H * d->dk);
  M3_REQUIRE(d->T <= 1 || d->ldp >= d->H * d->dk, "attention: ldp=%d is shorter than a row of %d", d->ldp, d->H * d->dk);
  M3_REQUIRE(aligned16(d->qkv) && aligned16(d->p) && aligned16(d->out), "attention: qkv / p / out must be 16-byte aligned");
  q->qkv = d->qkv; q->ldq = d->ldq; q->pmat = d->p; q->ldp = d->ldp; q->pos_u = d->pos_u; q->pos_v = d->pos_v; q->row_len = d->len;
  q->B = d->B; q->T = d->T; q->H = d->H; q->dk = d->dk; q->scale = d->scale; q->out = d->out; q->ldo = d->ldo; q->chunk = d->chunk;
  q->left_chunks = d->left_chunks;
  return 0;
}
static int attention_single(const void* qkv, int ldq, const float* p, int ldp, const float* pos_u, const float* pos_v, const int32_t* len, int B, int T,
                            int H, int dk, float scale, int chunk, int left_chunks, void* out, int ldo, int rows_bf16, m3_stream stream) {
  const m3_attention_desc d = {(const float*)qkv, ldq, p, ldp, pos_u, pos_v, len, B, T, H, dk, scale, chunk, left_chunks, (float*)out, ldo};
  AttArgs a;
  if (int rc = attention_args_from_desc(&d, "attention", -1, &a)) return rc;
  a.rows_bf16 = rows_bf16;
  return launch_relpos_attention(a, (hipStream_t)stream);
}

static int linear_params(const m3_linear_desc* d, GemmParams* out) {
  M3_REQUIRE(d != nullptr, "linear: null descriptor");
  GemmParams p;
  p.A = d->a; p.lda = d->lda;
  p.A2 = d->a2; p.lda2 = d->lda2; p.K1 = d->k1;
  p.mode = d->a2 ? GEMM_A_CONCAT2 : GEMM_A_PLAIN;
  p.W = (const float*)d->w; p.bias = d->bias; p.Y = d->y; p.ldy = d->ldy;
  M3_REQUIRE(d->weight_dtype == M3_F32 || d->weight_dtype == M3_BF16, "linear: weight_dtype %d", d->weight_dtype);
  p.w_bf16 = d->weight_dtype == M3_BF16;
  p.M = d->M; p.N = d->N; p.K = d->K;
  p.ln_gamma = d->ln_gamma; p.ln_beta = d->ln_beta; p.ln_eps = d->ln_eps;
  p.ln_wsum = d->ln_wsum; p.ln_wbeta = d->ln_wbeta;
  p.row_len = d->len; p.rows_per_batch = d->rows_per_batch; p.mask_in = d->mask_in; p.mask_out = d->mask_out;
  p.act = d->act; p.alpha = d->alpha; p.resid = d->resid; p.ldr = d->ldr;
  M3_REQUIRE((d->a_dtype == M3_F32 || d->a_dtype == M3_BF16) && (d->y_dtype == M3_F32 || d->y_dtype == M3_BF16),
             "linear: a_dtype / y_dtype must be f32 or bf16");
  if (d->a_dtype == M3_BF16 || d->y_dtype == M3_BF16 || d->y_copy_bf16)
    M3_REQUIRE(p.w_bf16 && p.mode == GEMM_A_PLAIN && !p.ln_gamma, "linear: bf16 activations need bf16 weights, plain A, no affine LayerNorm");
  p.a_bf16 = d->a_dtype == M3_BF16; p.y_bf16 = d->y_dtype == M3_BF16;
  p.Yb = d->y_copy_bf16; p.ldyb = d->ld_copy; p.Yb_stats = d->y_copy_stats;
  p.ln_stats = d->ln_stats; p.ln_stat_parts = d->ln_stat_parts;
  // Row strides (include/m3asr.h).  Multiples: the 16-byte loads of `a` / `a2` and the 8-byte stores of bf16 rows need them (the
  // fp32 `y` / `resid` paths fall back to element accesses on other strides).  Minimum: rows of an operand may not overlap.
  {
    const int n_out = d->act == M3_ACT_GLU ? d->N / 2 : d->N;
    const int k1 = d->a2 ? d->k1 : d->K, a_mult = p.a_bf16 ? 8 : 4;
    const bool rows = d->M > 1;   // with one row a stride is never used
    M3_REQUIRE(d->lda % a_mult == 0 && (!rows || d->lda >= k1), "linear: lda=%d must be a multiple of %d and >= %d", d->lda, a_mult, k1);
    if (d->a2) M3_REQUIRE(d->lda2 % 4 == 0 && (!rows || d->lda2 >= d->K - k1), "linear: lda2=%d must be a multiple of 4 and >= %d", d->lda2, d->K - k1);
    M3_REQUIRE(!rows || d->ldy >= n_out, "linear: ldy=%d is shorter than an output row of %d", d->ldy, n_out);
    if (p.y_bf16) M3_REQUIRE(d->ldy % 4 == 0, "linear: ldy=%d must be a multiple of 4 for a bf16 y", d->ldy);
    if (d->resid) M3_REQUIRE(!rows || d->ldr >= n_out, "linear: ldr=%d is shorter than an output row of %d", d->ldr, n_out);
    if (d->y_copy_bf16) M3_REQUIRE(d->ld_copy % 4 == 0 && (!rows || d->ld_copy >= n_out), "linear: ld_copy=%d must be a multiple of 4 and >= %d", d->ld_copy, n_out);
  }
  *out = p;
  return 0;
}
// the operands a launch dereferences (m3_linear_workspace_size only reads sizes): rows accessed 16 bytes at a time start on a
// 16-byte boundary, and an in-place residual update walks y and resid with one stride
static int linear_pointers(const m3_linear_desc* d) {
  M3_REQUIRE(d->a && d->w && d->y, "linear: null a / w / y");
  M3_REQUIRE(aligned16(d->a) && aligned16(d->a2) && aligned16(d->y) && aligned16(d->resid) && aligned16(d->y_copy_bf16),
             "linear: a / a2 / y / resid / y_copy_bf16 must be 16-byte aligned");
  M3_REQUIRE((const void*)d->resid != (const void*)d->y || d->ldr == d->ldy, "linear: y == resid (in-place) needs ldr=%d == ldy=%d", d->ldr, d->ldy);
  return 0;
}
const char* m3_linear_kernel(const m3_linear_desc* d, int with_workspace) {
  GemmParams p;
  if (linear_params(d, &p)) return nullptr;
  const GemmPlan plan = plan_gemm(p, with_workspace ? SIZE_MAX : 0);
  if (plan.launches == 0) set_error("%s", plan.reason);
  return plan.launches ? plan.label : nullptr;
}
int m3_linear(const m3_linear_desc* d, m3_stream stream) { return m3_linear_ws(d, nullptr, 0, stream); }
size_t m3_linear_workspace_size(const m3_linear_desc* d) {
  GemmParams p;
  return linear_params(d, &p) == 0 ? plan_gemm(p, SIZE_MAX).ws_bytes : 0;
}
// (a missing or too-small workspace: the plan is the one-launch form)
int m3_linear_ws(const m3_linear_desc* d, void* workspace, size_t workspace_bytes, m3_stream stream) {
  GemmParams p;
  if (int rc = linear_params(d, &p)) return rc;
  if (int rc = linear_pointers(d)) return rc;
  return launch_gemm(gemm_launch(p, (float*)workspace, workspace_bytes), (hipStream_t)stream);
}
// desc->w in fragment order (m3_pack_wfrag_host): the plan takes it on the skinny fp32 kernel alone and refuses the rest
int m3_linear_wfrag(const m3_linear_desc* d, m3_stream stream) {
  GemmParams p;
  if (int rc = linear_params(d, &p)) return rc;
  if (int rc = linear_pointers(d)) return rc;
  M3_REQUIRE(aligned16(d->w), "linear: fragment-ordered w must be 16-byte aligned");
  p.w_frag = 1;
  return launch_gemm(gemm_launch(p, nullptr, 0), (hipStream_t)stream);
}
const char* m3_linear_wfrag_kernel(const m3_linear_desc* d) {
  GemmParams p;
  if (linear_params(d, &p)) return nullptr;
  p.w_frag = 1;
  const GemmPlan plan = plan_gemm(p, 0);
  if (plan.launches == 0) set_error("%s", plan.reason);
  return plan.launches ? plan.label : nullptr;
}
int m3_pack_wfrag_host(const float* w, int N, int K, float* wf) {
  M3_REQUIRE(w != nullptr && wf != nullptr && N > 0 && K > 0 && N % 16 == 0 && K % 16 == 0,
             "pack_wfrag: N=%d and K=%d must be positive multiples of 16", N, K);
  const int nsteps = K / 16;
  for (int nt = 0; nt < N / 16; ++nt)
    for (int s = 0; s < nsteps; ++s)
      for (int kq = 0; kq < 4; ++kq)
        for (int col = 0; col < 16; ++col)
          for (int j = 0; j < 4; ++j)
            wf[((((size_t)nt * nsteps + s) * 4 + kq) * 16 + col) * 4 + j] = w[(size_t)(16 * nt + col) * K + 16 * s + 4 * kq + j];
  return 0;
}

int m3_layer_norm(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int dim,
                  m3_stream stream) {
  return launch_layernorm(x, gamma, beta, eps, y, rows, dim, (hipStream_t)stream);
}
int m3_relpos_attention(const float* qkv, int ldq, const float* p, int ldp, const float* pos_u, const float* pos_v,
                        const int32_t* len, int B, int T, int H, int dk, float scale, float* out, int ldo,
                        m3_stream stream) {
  return attention_single(qkv, ldq, p, ldp, pos_u, pos_v, len, B, T, H, dk, scale, 0, -1, out, ldo, 0, stream);
}
int m3_relpos_attention_bf16(const void* qkv, int ldq, const float* p, int ldp, const float* pos_u, const float* pos_v,
                             const int32_t* len, int B, int T, int H, int dk, float scale, int chunk, int left_chunks,
                             void* out, int ldo, m3_stream stream) {
  return attention_single(qkv, ldq, p, ldp, pos_u, pos_v, len, B, T, H, dk, scale, chunk, left_chunks, out, ldo, 1, stream);
}
int m3_relpos_attention_chunk(const float* qkv, int ldq, const float* p, int ldp, const float* pos_u, const float* pos_v,
                              const int32_t* len, int B, int T, int H, int dk, float scale, int chunk, int left_chunks,
                              float* out, int ldo, m3_stream stream) {
  return attention_single(qkv, ldq, p, ldp, pos_u, pos_v, len, B, T, H, dk, scale, chunk, left_chunks, out, ldo, 0, stream);
}
// The depthwise conv at the boundary: the record from the ABI descriptor plus what only the boundary asks.  pair < 0: a single entry
// (`who` in its messages), which takes an empty batch as a launch of nothing; pair = 0 / 1: a problem of m3_dwconv_ln_silu_pair.
// zname: what the entry calls z.  strict: the entry asks for 16-byte aligned operands and for gamma and beta together
// (m3_dwconv_ln_silu, the oldest entry, never did: it refuses only what the kernel would dereference as a null pointer).
static int dwconv_args_from_desc(const m3_dwconv_desc* d, const char* who, const char* zname, int pair, bool strict, DwArgs* q) {
  if (pair >= 0) M3_REQUIRE(d->B > 0 && d->T > 0 && d->D > 0 && d->K > 0, "%s: empty problem %d", who, pair);
  const bool ln_ok = strict ? (d->gamma == nullptr) == (d->beta == nullptr) : (d->gamma == nullptr || d->beta != nullptr);
  M3_REQUIRE((pair < 0 && (d->B <= 0 || d->T <= 0)) || (d->z && d->w_kc && d->bias && d->out && ln_ok),
             "%s: null %s / w_kc / bias / out, or gamma without beta", who, zname);
  M3_REQUIRE(!strict || (aligned16(d->z) && aligned16(d->w_kc) && aligned16(d->bias) && aligned16(d->gamma) && aligned16(d->beta) &&
                          aligned16(d->left_fill) && aligned16(d->out)), "%s: every operand must be 16-byte aligned", who);
  if (pair >= 0) {   // (a single entry has no gate_sigmoided, and hears the launcher's words about K)
    M3_REQUIRE(d->ldz >= 0 && (d->ldz > 0 || !d->gate_sigmoided), "%s: ldz=%d (sigmoided gate columns belong to the GLU-on-load form)", who, d->ldz);
    M3_REQUIRE(d->left_fill == nullptr || d->K >= 2, "%s: the causal conv needs K >= 2", who);
  }
  q->z = d->z; q->glu_ldz = d->ldz; q->glu_sig = d->gate_sigmoided != 0; q->w_kc = d->w_kc; q->bias = d->bias; q->gamma = d->gamma;
  q->beta = d->beta; q->eps = d->eps; q->causal_left_fill = d->left_fill; q->B = d->B; q->T = d->T; q->D = d->D; q->K = d->K; q->out = d->out;
  return 0;
}
static m3_dwconv_desc dwconv_desc(const float* z, int ldz, const float* w_kc, const float* bias, const float* gamma, const float* beta, float eps,
                                  const float* left_fill, int B, int T, int D, int K, float* out) {
  return m3_dwconv_desc{z, ldz, 0, w_kc, bias, gamma, beta, eps, left_fill, B, T, D, K, out};
}
int m3_dwconv_ln_silu(const float* z, const float* w_kc, const float* bias, const float* gamma, const float* beta,
                      float eps, int B, int T, int D, int K, float* out, m3_stream stream) {
  const m3_dwconv_desc d = dwconv_desc(z, 0, w_kc, bias, gamma, beta, eps, nullptr, B, T, D, K, out);
  DwArgs a;
  if (int rc = dwconv_args_from_desc(&d, "dwconv", "z", -1, false, &a)) return rc;
  return launch_dwconv_ln_silu(a, (hipStream_t)stream);
}
int m3_dwconv_glu_ln_silu(const float* vg, int ldz, const float* w_kc, const float* bias, const float* gamma, const float* beta,
                          float eps, int B, int T, int D, int K, float* out, m3_stream stream) {
  M3_REQUIRE(B > 0 && T > 0, "dwconv (GLU on load): empty problem");
  const m3_dwconv_desc d = dwconv_desc(vg, ldz, w_kc, bias, gamma, beta, eps, nullptr, B, T, D, K, out);
  DwArgs a;
  if (int rc = dwconv_args_from_desc(&d, "dwconv (GLU on load)", "vg", -1, true, &a)) return rc;
  M3_REQUIRE(ldz > 0, "dwconv (GLU on load): ldz=%d", ldz);
  return launch_dwconv_ln_silu(a, (hipStream_t)stream);
}
// The stateful launches of the chunk-by-chunk engine (engine.hip "att_stream" / "conv.dw_ln_silu" stages) at the boundary: argument
// checks and one launcher call each.  What lives on the device (the counters, chunk_len) cannot be checked here.
int m3_relpos_attention_stream(const float* qkv, int ldq, float* hist, int cap, const float* p, int ldp, int p_rows, const float* pos_u,
                               const float* pos_v, const int32_t* chunk_len, const int32_t* step, int B, int C, int H, int dk,
                               float scale, int left_chunks, int slot_max_chunks, float* out, int ldo, m3_stream stream) {
  M3_REQUIRE(B > 0 && C > 0 && H > 0 && dk > 0, "attention (stream): empty problem");
  M3_REQUIRE(qkv && p && pos_u && pos_v && out, "attention (stream): null qkv / p / pos_u / pos_v / out");
  M3_REQUIRE(ldq >= 3 * H * dk && ldp >= H * dk && ldo >= H * dk, "attention (stream): ldq=%d / ldp=%d / ldo=%d shorter than the rows (%d / %d / %d)",
             ldq, ldp, ldo, 3 * H * dk, H * dk, H * dk);
  M3_REQUIRE(aligned16(qkv) && aligned16(hist) && aligned16(p) && aligned16(pos_u) && aligned16(pos_v) && aligned16(out),
             "attention (stream): qkv / hist / p / pos_u / pos_v / out must be 16-byte aligned");
  M3_REQUIRE(p_rows >= C, "attention (stream): a position table of %d rows is shorter than one chunk of %d", p_rows, C);
  M3_REQUIRE(slot_max_chunks < 0 || (long)slot_max_chunks * C <= (long)p_rows,
             "attention (stream, slot mode): %d chunks of %d frames pass the position table's %d rows", slot_max_chunks, C, p_rows);
  AttArgs a;
  a.qkv = qkv; a.ldq = ldq; a.pmat = p; a.ldp = ldp; a.pos_u = pos_u; a.pos_v = pos_v; a.row_len = chunk_len; a.B = B; a.T = C; a.H = H; a.dk = dk;
  a.scale = scale; a.out = out; a.ldo = ldo; a.left_chunks = left_chunks;
  a.streaming = 1; a.hist = hist; a.cap = cap; a.step = step; a.slot_max_chunks = slot_max_chunks;
  return launch_relpos_attention(a, (hipStream_t)stream);
}
int m3_dwconv_ln_silu_stream(const float* z, const float* w_kc, const float* bias, const float* gamma, const float* beta, float eps, int B,
                             int T, int D, int K, float* cache_pair, const int32_t* step, const int32_t* chunk_len, int slot_max_chunks,
                             float* out, m3_stream stream) {
  M3_REQUIRE(B > 0 && T > 0 && D > 0, "dwconv (stream): empty problem");
  const m3_dwconv_desc d = dwconv_desc(z, 0, w_kc, bias, gamma, beta, eps, nullptr, B, T, D, K, out);
  DwArgs a;
  if (int rc = dwconv_args_from_desc(&d, "dwconv (stream)", "z", -1, true, &a)) return rc;
  M3_REQUIRE(aligned16(cache_pair), "dwconv (stream): every operand must be 16-byte aligned");
  a.streaming = 1; a.cache_pair = cache_pair; a.step = step; a.chunk_len = chunk_len; a.slot_max_chunks = slot_max_chunks;
  return launch_dwconv_ln_silu(a, (hipStream_t)stream);
}
int m3_dwconv_ln_silu_causal(const float* z, const float* w_kc, const float* bias, const float* gamma, const float* beta, float eps,
                             const float* left_fill, int B, int T, int D, int K, float* out, m3_stream stream) {
  const m3_dwconv_desc d = dwconv_desc(z, 0, w_kc, bias, gamma, beta, eps, left_fill, B, T, D, K, out);
  DwArgs a;
  M3_REQUIRE(left_fill != nullptr, "dwconv (causal): left_fill [D], the frame left of frame 0, must be supplied");
  if (int rc = dwconv_args_from_desc(&d, "dwconv (causal)", "z", -1, true, &a)) return rc;
  return launch_dwconv_ln_silu(a, (hipStream_t)stream);
}
// The first conv at the boundary: the record from the ABI descriptor plus what only the boundary asks.  pair < 0: a single entry
// (`who` in its messages), which takes an empty batch as a launch of nothing; pair = 0 / 1: a problem of m3_subsample_conv1_pair.
static int conv1_args_from_desc(const m3_conv1_ch_desc* d, const char* who, int pair, Conv1Args* q) {
  M3_REQUIRE(d->in_ch >= 1 && d->in_ch <= 3, "%s: in_ch=%d outside [1, 3]", who, d->in_ch);
  M3_REQUIRE(d->idim % d->in_ch == 0, "%s: idim=%d is no multiple of in_ch=%d", who, d->idim, d->in_ch);
  M3_REQUIRE((pair < 0 && d->B <= 0) || (d->feat && d->w9c && d->bias && d->out), "%s: null feat / w9c / bias / out", who);
  M3_REQUIRE(d->act == M3_ACT_NONE || d->act == M3_ACT_RELU, "%s: act %d (none / relu)", who, d->act);
  M3_REQUIRE((d->cmvn_mean == nullptr) == (d->cmvn_istd == nullptr), "%s: cmvn mean and istd go together", who);
  M3_REQUIRE((d->feat_len == nullptr) == (d->lens_out == nullptr) && (pair <= 0 || d->feat_len == nullptr),
             "%s: feat_len and lens_out go together, on the first problem only", who);
  if (pair >= 0) {   // (the words of the pair entry; a single entry hears the launcher's)
    M3_REQUIRE(d->B > 0 && d->T >= 3 && d->idim / d->in_ch >= 3, "%s: input (B=%d, T=%d, idim=%d) shorter than the 3x3 kernel", who, d->B, d->T,
               d->idim / d->in_ch);
    M3_REQUIRE(d->C > 0 && (d->C & 3) == 0 && d->C <= 1024, "%s: channels=%d must be a multiple of 4 (<= 1024)", who, d->C);
  }
  q->feat = d->feat; q->w9c = d->w9c; q->bias = d->bias; q->cmvn_mean = d->cmvn_mean; q->cmvn_istd = d->cmvn_istd;
  q->B = d->B; q->T = d->T; q->idim = d->idim; q->C = d->C; q->out = d->out; q->relu = d->act == M3_ACT_RELU;
  q->feat_len = d->feat_len; q->lens_out = d->lens_out; q->in_ch = d->in_ch; q->out_bf16 = d->out_bf16 != 0;
  return 0;
}
// the one-channel descriptor as the record's: in_ch = 1, fp32 out
static m3_conv1_ch_desc conv1_ch_desc(const m3_conv1_desc& d) {
  return {d.feat, d.w9c, d.bias, d.cmvn_mean, d.cmvn_istd, d.B, d.T, d.idim, d.C, d.act, d.out, d.feat_len, d.lens_out, 1, 0};
}
static int conv1_single(const char* who, const float* feat, const float* w9c, const float* bias, const float* cmvn_mean, const float* cmvn_istd,
                        int B, int T, int idim, int C, int act, float* out, m3_stream stream) {
  const m3_conv1_ch_desc d = {feat, w9c, bias, cmvn_mean, cmvn_istd, B, T, idim, C, act, out, nullptr, nullptr, 1, 0};
  Conv1Args q;
  if (int rc = conv1_args_from_desc(&d, who, -1, &q)) return rc;
  return launch_conv1_relu(q, (hipStream_t)stream);
}
int m3_subsample_conv1(const float* feat, const float* w9c, const float* bias, int B, int T, int idim, int C,
                       float* out, m3_stream stream) {
  return conv1_single("subsample_conv1", feat, w9c, bias, nullptr, nullptr, B, T, idim, C, M3_ACT_RELU, out, stream);
}
int m3_subsample_conv1_cmvn(const float* feat, const float* w9c, const float* bias, const float* cmvn_mean,
                            const float* cmvn_istd, int B, int T, int idim, int C, float* out, m3_stream stream) {
  return conv1_single("subsample_conv1", feat, w9c, bias, cmvn_mean, cmvn_istd, B, T, idim, C, M3_ACT_RELU, out, stream);
}
int m3_subsample_conv1_ch(const m3_conv1_ch_desc* d, m3_stream stream) {
  M3_REQUIRE(d != nullptr, "subsample_conv1_ch: null descriptor");
  Conv1Args q;
  if (int rc = conv1_args_from_desc(d, "subsample_conv1_ch", -1, &q)) return rc;
  return launch_conv1_relu(q, (hipStream_t)stream);
}
int m3_conv2d_3x3s2_first(const float* feat, const float* w9c, const float* bias, int B, int T, int idim, int C, int act,
                          float* out, m3_stream stream) {
  return conv1_single("conv2d", feat, w9c, bias, nullptr, nullptr, B, T, idim, C, act, out, stream);
}
int m3_cmvn(const float* x, const int32_t* len, const float* mean, const float* istd, int B, int T, int D, float* y,
            m3_stream stream) {
  M3_REQUIRE(x && mean && istd && y, "cmvn: null pointer");
  return launch_cmvn(x, len, mean, istd, B, T, D, y, (hipStream_t)stream);
}
int m3_log_softmax_bias(const float* x, const float* bias, float* y, size_t rows, int n, m3_stream stream) {
  M3_REQUIRE(x && y && n > 0, "log_softmax_bias: bad arguments");
  return launch_log_softmax_bias(x, bias, y, rows, n, (hipStream_t)stream);
}
int m3_subsample_conv2(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C, float* out,
                       m3_stream stream) {
  return m3_conv2d_3x3s2(in, w, bias, B, T1, F1, C, M3_ACT_RELU, out, stream);
}
static int conv2d_params(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C, int act, float* out, GemmParams* q) {
  M3_REQUIRE(T1 >= 3 && F1 >= 3, "subsample_conv2: input (%d,%d) smaller than the kernel", T1, F1);
  M3_REQUIRE(act == M3_ACT_NONE || act == M3_ACT_RELU || act == M3_ACT_SILU, "conv2d: act %d", act);
  GemmParams p;
  p.mode = GEMM_A_CONV3X3S2;
  p.A = in; p.lda = 4;
  p.conv_T1 = T1; p.conv_F1 = F1; p.conv_T2 = (T1 - 3) / 2 + 1; p.conv_F2 = (F1 - 3) / 2 + 1; p.conv_C = C;
  p.W = w; p.bias = bias; p.Y = out; p.ldy = C;
  p.M = B * p.conv_T2 * p.conv_F2; p.N = C; p.K = 9 * C;
  p.act = act;
  *q = p;
  return 0;
}
int m3_conv2d_3x3s2(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C, int act, float* out,
                    m3_stream stream) {
  return m3_conv2d_3x3s2_ws(in, w, bias, B, T1, F1, C, act, out, nullptr, 0, stream);
}
size_t m3_conv2d_3x3s2_workspace_size(int B, int T1, int F1, int C, int act) {
  GemmParams p;
  return conv2d_params(nullptr, nullptr, nullptr, B, T1, F1, C, act, nullptr, &p) == 0 ? plan_gemm(p, SIZE_MAX).ws_bytes : 0;
}
// (a missing or too-small workspace: the plan is the one-launch form)
int m3_conv2d_3x3s2_ws(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C, int act, float* out,
                       void* workspace, size_t workspace_bytes, m3_stream stream) {
  GemmParams p;
  if (int rc = conv2d_params(in, w, bias, B, T1, F1, C, act, out, &p)) return rc;
  return launch_gemm(gemm_launch(p, (float*)workspace, workspace_bytes), (hipStream_t)stream);
}

// ---- the packed-row and bf16-row operand forms at the boundary (include/m3asr.h): the record the engine fills, checked as the
// single entry of the operator checks it, one launcher call
static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
int m3_pack_plan(int32_t* len, int B, int T, int32_t* row0, int32_t* pad_of, const int32_t* feat_len, m3_stream stream) {
  M3_REQUIRE(len && row0 && pad_of, "pack_plan: null len / row0 / pad_of");
  M3_REQUIRE(aligned4(len) && aligned4(row0) && aligned4(pad_of) && aligned4(feat_len), "pack_plan: every operand must be 4-byte aligned");
  return launch_pack_plan(len, B, T, row0, pad_of, (hipStream_t)stream, feat_len);
}
int m3_unpack_rows(const float* in, const int32_t* row0, int B, int T, int n, float* out, m3_stream stream) {
  M3_REQUIRE(B >= 0 && T >= 0 && n >= 1, "unpack_rows: bad sizes B=%d T=%d n=%d", B, T, n);
  M3_REQUIRE((long)B * T == 0 || (in && row0 && out), "unpack_rows: null in / row0 / out");
  M3_REQUIRE(aligned4(in) && aligned4(row0) && aligned4(out), "unpack_rows: every operand must be 4-byte aligned");
  return launch_unpack_rows(in, row0, B, T, n, out, (hipStream_t)stream);
}
int m3_linear_live_rows(const m3_linear_desc* d, const int32_t* live_rows_dev, void* workspace, size_t workspace_bytes, m3_stream stream) {
  GemmParams p;
  if (int rc = linear_params(d, &p)) return rc;
  if (int rc = linear_pointers(d)) return rc;
  M3_REQUIRE(live_rows_dev != nullptr && aligned4(live_rows_dev), "linear (live rows): live_rows_dev must be a 4-byte aligned device pointer");
  p.m_dev = live_rows_dev;
  return launch_gemm(gemm_launch(p, (float*)workspace, workspace_bytes), (hipStream_t)stream);
}
const char* m3_linear_live_rows_kernel(const m3_linear_desc* d, int with_workspace) { return m3_linear_kernel(d, with_workspace); }
int m3_moe_router_live_rows(const float* embed, int ld_embed, int embed_dim, const float* x, int ldx, int idim, const float* w,
                            const float* bias, const float* ln_gamma, const float* ln_beta, float ln_eps, float* xn, int ld_xn,
                            float* logits, int ld_logits, int S, int num_expert, const int32_t* live_rows_dev, m3_stream stream) {
  M3_REQUIRE(S <= 1 || (ld_embed >= embed_dim && ldx >= idim), "moe_router (live rows): ld_embed=%d / ldx=%d shorter than the rows (%d / %d)",
             ld_embed, ldx, embed_dim, idim);
  M3_REQUIRE(S <= 1 || xn == nullptr || ld_xn >= idim, "moe_router (live rows): ld_xn=%d is shorter than a row of %d", ld_xn, idim);
  M3_REQUIRE(S <= 1 || ld_logits >= num_expert, "moe_router (live rows): ld_logits=%d is shorter than a row of %d", ld_logits, num_expert);
  M3_REQUIRE(aligned16(embed) && aligned16(x) && aligned16(xn), "moe_router (live rows): embed / x / xn must be 16-byte aligned");
  M3_REQUIRE(live_rows_dev != nullptr && aligned4(live_rows_dev), "moe_router (live rows): live_rows_dev must be a 4-byte aligned device pointer");
  return launch_moe_router(embed, ld_embed, embed_dim, x, ldx, idim, w, bias, ln_gamma, ln_beta, ln_eps, xn, ld_xn, logits, ld_logits, S,
                           num_expert, live_rows_dev, (hipStream_t)stream);
}
static int conv2d_frames_params(const float* in, const void* w, const float* bias, int B, int T1, int F1, int C, int act, int w_bf16, float* out,
                                GemmParams* q) {
  M3_REQUIRE(B > 0 && C > 0, "conv2d (frames): empty problem B=%d C=%d", B, C);
  if (int rc = conv2d_params(in, (const float*)w, bias, B, T1, F1, C, act, out, q)) return rc;
  q->w_bf16 = w_bf16 != 0;
  return 0;
}
int m3_conv2d_3x3s2_frames(const float* in, const void* w, const float* bias, int B, int T1, int F1, int C, int act,
                           const int32_t* frames_dev, int w_bf16, float* out, m3_stream stream) {
  GemmParams p;
  if (int rc = conv2d_frames_params(in, w, bias, B, T1, F1, C, act, w_bf16, out, &p)) return rc;
  M3_REQUIRE(in && w && out, "conv2d (frames): null in / w / out");
  M3_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out) && aligned4(frames_dev), "conv2d (frames): in / w / out must be 16-byte, frames_dev 4-byte aligned");
  p.conv_len = frames_dev;
  return launch_gemm(gemm_launch(p, nullptr, 0), (hipStream_t)stream);
}
const char* m3_conv2d_3x3s2_kernel(int B, int T1, int F1, int C, int act, int w_bf16, int with_workspace) {
  GemmParams p;
  if (conv2d_frames_params(nullptr, nullptr, nullptr, B, T1, F1, C, act, w_bf16, nullptr, &p)) return nullptr;
  const GemmPlan plan = plan_gemm(p, with_workspace ? SIZE_MAX : 0);
  if (plan.launches == 0) set_error("%s", plan.reason);
  return plan.launches ? plan.label : nullptr;
}
static int attention_packed(const char* who, const m3_attention_desc* d, const int32_t* row0, int out_bf16, int rows_bf16, m3_stream stream) {
  M3_REQUIRE(d != nullptr, "%s: null descriptor", who);
  M3_REQUIRE(d->B > 0 && d->T > 0 && d->H > 0 && d->dk > 0, "%s: empty problem", who);
  AttArgs a;
  if (int rc = attention_args_from_desc(d, who, -1, &a)) return rc;
  M3_REQUIRE(row0 == nullptr || d->len != nullptr, "%s: packed rows (row0) need len", who);
  M3_REQUIRE(aligned4(row0) && aligned4(d->len), "%s: row0 / len must be 4-byte aligned", who);
  a.row0 = row0; a.out_bf16 = out_bf16 != 0; a.rows_bf16 = rows_bf16;
  return launch_relpos_attention(a, (hipStream_t)stream);
}
int m3_relpos_attention_packed(const m3_attention_desc* d, const int32_t* row0, int out_bf16, m3_stream stream) {
  return attention_packed("attention (packed)", d, row0, out_bf16, 0, stream);
}
int m3_relpos_attention_bf16_packed(const m3_attention_desc* d, const int32_t* row0, m3_stream stream) {
  return attention_packed("attention (bf16 rows, packed)", d, row0, 0, 1, stream);
}
int m3_dwconv_ln_silu_packed(const m3_dwconv_desc* d, const int32_t* pad_of, const int32_t* row0, const int32_t* row_len, int out_bf16,
                             m3_stream stream) {
  M3_REQUIRE(d != nullptr, "dwconv (packed): null descriptor");
  DwArgs a;
  if (int rc = dwconv_args_from_desc(d, "dwconv (packed)", "z", 0, true, &a)) return rc;
  M3_REQUIRE((pad_of != nullptr) == (row0 != nullptr) && (pad_of != nullptr) == (row_len != nullptr),
             "dwconv (packed): pad_of, row0 and row_len go together (all three, or none for the padded layout)");
  M3_REQUIRE(aligned4(pad_of) && aligned4(row0) && aligned4(row_len), "dwconv (packed): pad_of / row0 / row_len must be 4-byte aligned");
  a.pad_of = pad_of; a.row0 = row0; a.row_len = row_len; a.out_bf16 = out_bf16 != 0;
  return launch_dwconv_ln_silu(a, (hipStream_t)stream);
}
int m3_layer_norm_ex(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int dim, void* y_bf16,
                     float* y_stats, const float* gamma2, const float* beta2, float eps2, float* y2, m3_stream stream) {
  M3_REQUIRE(rows >= 0 && dim > 0, "layer_norm_ex: bad sizes rows=%d dim=%d", rows, dim);
  M3_REQUIRE(rows == 0 || (x && gamma && beta && y), "layer_norm_ex: null x / gamma / beta / y");
  M3_REQUIRE(y_stats == nullptr || y_bf16 != nullptr, "layer_norm_ex: y_stats are the statistics of y_bf16, which is null");
  M3_REQUIRE((gamma2 != nullptr) == (beta2 != nullptr) && (gamma2 != nullptr) == (y2 != nullptr),
             "layer_norm_ex: the second LayerNorm needs gamma2, beta2 and y2 (all three, or none)");
  M3_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y) && aligned16(y_bf16) && aligned16(y_stats) &&
             aligned16(gamma2) && aligned16(beta2) && aligned16(y2), "layer_norm_ex: every operand must be 16-byte aligned");
  return launch_layernorm(x, gamma, beta, eps, y, rows, dim, (hipStream_t)stream, y_bf16, y_stats, gamma2, beta2, eps2, y2);
}
int m3_row_stats_bf16(const void* xb, int rows, int dim, float* stats, m3_stream stream) {
  M3_REQUIRE(rows >= 0 && dim > 0, "row_stats_bf16: bad sizes rows=%d dim=%d", rows, dim);
  M3_REQUIRE(rows == 0 || (xb && stats), "row_stats_bf16: null xb / stats");
  M3_REQUIRE(aligned16(xb) && aligned16(stats), "row_stats_bf16: xb / stats must be 16-byte aligned");
  return launch_row_stats_bf16(xb, rows, dim, stats, (hipStream_t)stream);
}
int m3_rows_to_bf16(const float* x, int ldx, int S, int dim, void* xb, m3_stream stream) {
  M3_REQUIRE(S >= 0 && dim > 0, "rows_to_bf16: bad sizes S=%d dim=%d", S, dim);
  M3_REQUIRE(S == 0 || (x && xb), "rows_to_bf16: null x / xb");
  M3_REQUIRE(S <= 1 || ldx >= dim, "rows_to_bf16: ldx=%d is shorter than a row of %d", ldx, dim);
  M3_REQUIRE(aligned16(x) && (reinterpret_cast<uintptr_t>(xb) & 7) == 0, "rows_to_bf16: x must be 16-byte, xb 8-byte aligned");
  return launch_rows_to_bf16(x, ldx, S, dim, xb, (hipStream_t)stream);
}

// ---- the paired launches at the boundary (include/m3asr.h): both problems checked as their single entries check them, outputs
// apart, one launcher call
static bool ranges_overlap(const void* a, size_t bytes_a, const void* b, size_t bytes_b) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + bytes_b && b0 < a0 + bytes_a;
}
static size_t rows_bytes(long rows, long ld, long width) { return rows > 0 ? (size_t)((rows - 1) * ld + width) * sizeof(float) : 0; }
static size_t linear_out_bytes(const m3_linear_desc* d) { return rows_bytes(d->M, d->ldy, d->act == M3_ACT_GLU ? d->N / 2 : d->N); }
// why two plans have no common instantiation of gemm_f32_dual_kernel, as text (gemm_dual_fusable says only that)
static int linear_pair_plans(const GemmLaunch& a, const GemmLaunch& b) {
  const GemmPlan &pa = a.plan, &pb = b.plan;
  const GemmPlan* const plans[2] = {&pa, &pb};
  for (int i = 0; i < 2; ++i) {
    const GemmPlan& q = *plans[i];
    M3_REQUIRE(q.launches > 0, "%s", q.reason);
    M3_REQUIRE(q.kernel == GemmKernel::SkinnyF32 && q.launches == 1, "linear pair: problem %d runs %s: only the skinny fp32 kernel (gemm_f32_kernel) pairs", i, q.label);
    M3_REQUIRE(q.dual_ok,
               "linear pair: problem %d has %d-row tiles, %d waves, %d load group%s: the paired kernel takes 16-row tiles, 4 or 8 waves, one load "
               "group, plain a, no affine LayerNorm", i, 16 * q.mt, q.nw, q.nbuf, q.nbuf == 1 ? "" : "s");
  }
  M3_REQUIRE(gemm_dual_fusable(a, b), "linear pair: the problems differ in waves (%d / %d), folded LayerNorm (%d / %d) or GLU (%d / %d)",
             pa.nw, pb.nw, pa.ln != GEMM_LN_NONE, pb.ln != GEMM_LN_NONE, (int)pa.glu, (int)pb.glu);
  return 0;
}
// (m3_linear_pair_kernel asks about plans made against any workspace: the workspaces themselves are the launch's to check)
static int splitk_pair_plans(const char* who, const GemmPlan& pa, const GemmPlan& pb) {
  const GemmPlan* const plans[2] = {&pa, &pb};
  for (int i = 0; i < 2; ++i) {
    M3_REQUIRE(plans[i]->launches > 0, "%s", plans[i]->reason);
    M3_REQUIRE(plans[i]->kernel == GemmKernel::SplitKF32, "%s: problem %d is no split-K problem with its workspace (it runs %s)", who, i, plans[i]->label);
  }
  M3_REQUIRE(pa.conv == pb.conv, "%s: an implicit conv pairs with an implicit conv, a plain problem with a plain one", who);
  return 0;
}
static int splitk_pair_launch(const char* who, const GemmLaunch& a, const void* out_a, size_t out_bytes_a, const GemmLaunch& b, const void* out_b,
                              size_t out_bytes_b, int which, m3_stream stream) {
  M3_REQUIRE(which >= 1 && which <= 3, "%s: which=%d (1 the GEMM launch, 2 the reduce launch, 3 both)", who, which);
  if (int rc = splitk_pair_plans(who, a.plan, b.plan)) return rc;
  M3_REQUIRE(!ranges_overlap(a.ws, a.plan.ws_bytes, b.ws, b.plan.ws_bytes), "%s: each problem needs its own workspace", who);
  M3_REQUIRE(!ranges_overlap(out_a, out_bytes_a, out_b, out_bytes_b), "%s: the two outputs overlap", who);
  return launch_gemm_f32_splitk_dual(a, b, (hipStream_t)stream, which);
}
const char* m3_linear_pair_kernel(const m3_linear_desc* a, const m3_linear_desc* b, int with_workspace) {
  GemmParams pa, pb;
  if (linear_params(a, &pa) || linear_params(b, &pb)) return nullptr;
  const size_t ws = with_workspace ? SIZE_MAX : 0;
  const GemmLaunch qa{pa, plan_gemm(pa, ws)}, qb{pb, plan_gemm(pb, ws)};
  if (with_workspace) return splitk_pair_plans("linear pair (workspaces)", qa.plan, qb.plan) ? nullptr : "gemm_f32_splitk_dual_kernel";
  return linear_pair_plans(qa, qb) ? nullptr : "gemm_f32_dual_kernel";
}
int m3_linear_pair(const m3_linear_desc* a, const m3_linear_desc* b, m3_stream stream) {
  GemmParams pa, pb;
  if (int rc = linear_params(a, &pa)) return rc;
  if (int rc = linear_params(b, &pb)) return rc;
  if (int rc = linear_pointers(a)) return rc;
  if (int rc = linear_pointers(b)) return rc;
  const GemmLaunch qa = gemm_launch(pa, nullptr, 0), qb = gemm_launch(pb, nullptr, 0);
  if (int rc = linear_pair_plans(qa, qb)) return rc;
  M3_REQUIRE(!ranges_overlap(a->y, linear_out_bytes(a), b->y, linear_out_bytes(b)), "linear pair: the two outputs overlap");
  return launch_gemm_f32_dual(qa, qb, (hipStream_t)stream);
}
// both w in fragment order (gemm_dual_fusable: the two problems agree on the layout)
int m3_linear_pair_wfrag(const m3_linear_desc* a, const m3_linear_desc* b, m3_stream stream) {
  GemmParams pa, pb;
  if (int rc = linear_params(a, &pa)) return rc;
  if (int rc = linear_params(b, &pb)) return rc;
  if (int rc = linear_pointers(a)) return rc;
  if (int rc = linear_pointers(b)) return rc;
  M3_REQUIRE(aligned16(a->w) && aligned16(b->w), "linear pair: fragment-ordered w must be 16-byte aligned");
  pa.w_frag = pb.w_frag = 1;
  const GemmLaunch qa = gemm_launch(pa, nullptr, 0), qb = gemm_launch(pb, nullptr, 0);
  if (int rc = linear_pair_plans(qa, qb)) return rc;
  M3_REQUIRE(!ranges_overlap(a->y, linear_out_bytes(a), b->y, linear_out_bytes(b)), "linear pair: the two outputs overlap");
  return launch_gemm_f32_dual(qa, qb, (hipStream_t)stream);
}
int m3_linear_ws_pair(const m3_linear_desc* a, void* workspace_a, size_t bytes_a, const m3_linear_desc* b, void* workspace_b,
                      size_t bytes_b, int which, m3_stream stream) {
  GemmParams pa, pb;
  if (int rc = linear_params(a, &pa)) return rc;
  if (int rc = linear_params(b, &pb)) return rc;
  if (int rc = linear_pointers(a)) return rc;
  if (int rc = linear_pointers(b)) return rc;
  return splitk_pair_launch("linear pair (workspaces)", gemm_launch(pa, (float*)workspace_a, bytes_a), a->y, linear_out_bytes(a),
                            gemm_launch(pb, (float*)workspace_b, bytes_b), b->y, linear_out_bytes(b), which, stream);
}
int m3_conv2d_3x3s2_ws_pair(const m3_conv2d_desc* a, void* workspace_a, size_t bytes_a, const m3_conv2d_desc* b, void* workspace_b,
                            size_t bytes_b, int which, m3_stream stream) {
  M3_REQUIRE(a != nullptr && b != nullptr, "conv2d pair: null descriptor");
  GemmParams pa, pb;
  if (int rc = conv2d_params(a->in, a->w, a->bias, a->B, a->T1, a->F1, a->C, a->act, a->out, &pa)) return rc;
  if (int rc = conv2d_params(b->in, b->w, b->bias, b->B, b->T1, b->F1, b->C, b->act, b->out, &pb)) return rc;
  M3_REQUIRE(a->in && a->w && a->out && b->in && b->w && b->out, "conv2d pair: null in / w / out");
  return splitk_pair_launch("conv2d pair", gemm_launch(pa, (float*)workspace_a, bytes_a), a->out, rows_bytes(pa.M, pa.ldy, pa.N),
                            gemm_launch(pb, (float*)workspace_b, bytes_b), b->out, rows_bytes(pb.M, pb.ldy, pb.N), which, stream);
}
int m3_relpos_attention_pair(const m3_attention_desc* a, const m3_attention_desc* b, m3_stream stream) {
  M3_REQUIRE(a != nullptr && b != nullptr, "attention pair: null descriptor");
  AttArgs qa, qb;
  if (int rc = attention_args_from_desc(a, "attention pair", 0, &qa)) return rc;
  if (int rc = attention_args_from_desc(b, "attention pair", 1, &qb)) return rc;
  M3_REQUIRE(relpos_attention_dual_fusable(qa, qb),
             "attention pair: head widths %d / %d (64 or 128 each) or row strides ldq %d / %d, ldp %d / %d (multiples of 4) are not a paired instantiation",
             a->dk, b->dk, a->ldq, b->ldq, a->ldp, b->ldp);
  M3_REQUIRE(!ranges_overlap(a->out, rows_bytes((long)a->B * a->T, a->ldo, a->H * a->dk), b->out, rows_bytes((long)b->B * b->T, b->ldo, b->H * b->dk)),
             "attention pair: the two outputs overlap");
  return launch_relpos_attention_dual(qa, qb, (hipStream_t)stream);
}
int m3_dwconv_ln_silu_pair(const m3_dwconv_desc* a, const m3_dwconv_desc* b, m3_stream stream) {
  M3_REQUIRE(a != nullptr && b != nullptr, "dwconv pair: null descriptor");
  DwArgs qa, qb;
  if (int rc = dwconv_args_from_desc(a, "dwconv pair", "z", 0, true, &qa)) return rc;
  if (int rc = dwconv_args_from_desc(b, "dwconv pair", "z", 1, true, &qb)) return rc;
  M3_REQUIRE(dwconv_dual_fusable(qa, qb),
             "dwconv pair: channels %d / %d, taps %d / %d, causal %d / %d, GLU on load (ldz) %d / %d: the problems must agree in each (D %% 4 == 0, "
             "<= 4096; symmetric: K odd; GLU on load: symmetric, K <= 15, 256 <= D <= 1024, ldz >= 2 D a multiple of 4)",
             a->D, b->D, a->K, b->K, a->left_fill != nullptr, b->left_fill != nullptr, a->ldz, b->ldz);
  M3_REQUIRE(!ranges_overlap(a->out, (size_t)a->B * a->T * a->D * 4, b->out, (size_t)b->B * b->T * b->D * 4), "dwconv pair: the two outputs overlap");
  return launch_dwconv_ln_silu_dual(qa, qb, (hipStream_t)stream);
}
static int conv1_pair(const m3_conv1_ch_desc* a, const m3_conv1_ch_desc* b, m3_stream stream) {
  Conv1Args qa, qb;
  if (int rc = conv1_args_from_desc(a, "conv1 pair", 0, &qa)) return rc;
  if (int rc = conv1_args_from_desc(b, "conv1 pair", 1, &qb)) return rc;
  auto bytes = [](const m3_conv1_ch_desc* d) {
    return (size_t)d->B * ((d->T - 3) / 2 + 1) * ((d->idim / d->in_ch - 3) / 2 + 1) * d->C * (d->out_bf16 ? 2 : sizeof(float));
  };
  M3_REQUIRE(a->B == b->B && a->T == b->T && a->idim == b->idim, "conv1 pair: the two problems do not share an input shape (B %d / %d, T %d / %d, idim %d / %d)",
             a->B, b->B, a->T, b->T, a->idim, b->idim);
  M3_REQUIRE(a->in_ch == b->in_ch, "conv1 pair: the two problems do not share in_ch (%d / %d); run them as two launches", a->in_ch, b->in_ch);
  M3_REQUIRE(!ranges_overlap(a->out, bytes(a), b->out, bytes(b)), "conv1 pair: the two outputs overlap");
  return launch_conv1_relu_dual(qa, qb, (hipStream_t)stream);
}
int m3_subsample_conv1_pair(const m3_conv1_desc* a, const m3_conv1_desc* b, m3_stream stream) {
  M3_REQUIRE(a != nullptr && b != nullptr, "conv1 pair: null descriptor");
  const m3_conv1_ch_desc ca = conv1_ch_desc(*a), cb = conv1_ch_desc(*b);
  return conv1_pair(&ca, &cb, stream);
}
int m3_subsample_conv1_ch_pair(const m3_conv1_ch_desc* a, const m3_conv1_ch_desc* b, m3_stream stream) {
  M3_REQUIRE(a != nullptr && b != nullptr, "conv1 pair: null descriptor");
  return conv1_pair(a, b, stream);
}

int m3_att_masked_softmax(const float* scores, const int32_t* len, int B, int H, int T1, int T2, float scale,
                          float* out, m3_stream stream) {
  return launch_att_masked_softmax(scores, len, B, H, T1, T2, scale, out, (hipStream_t)stream);
}
int m3_ctc_greedy(const float* logits, const int32_t* len, int B, int T, int V, int blank, int32_t* frame_ids,
                  int32_t* tokens, int32_t* n_tokens, m3_stream stream) {
  return launch_ctc_greedy(logits, len, B, T, V, blank, frame_ids, tokens, n_tokens, (hipStream_t)stream);
}
int m3_ctc_topk(const float* logits, size_t rows, int V, int k, float* top_logp, int32_t* top_idx, m3_stream stream) {
  return launch_ctc_topk(logits, rows, V, k, top_logp, top_idx, (hipStream_t)stream);
}
int m3_ctc_prefix_beam_search(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                              int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, int32_t* n_hyps) {
  return ctc_prefix_beam_search_host(top_logp, top_idx, T, k, beam, blank, hyp_tokens, hyp_len, hyp_score, n_hyps);
}
// ---- the device prefix beam search: plain, biased (ctx), fused (lm)
size_t m3_ctc_beam_state_size(const m3_ctc_beam_desc* desc) { return beam_state_need(desc, BeamForm::Plain); }
size_t m3_ctc_beam_ctx_state_size(const m3_ctc_beam_desc* desc) { return beam_state_need(desc, BeamForm::Ctx); }
size_t m3_ctc_beam_lm_state_size(const m3_ctc_beam_desc* desc) { return beam_state_need(desc, BeamForm::Lm); }
int m3_ctc_beam_reset(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, m3_stream stream) {
  return beam_reset(beam_call("ctc_beam_reset", BeamForm::Plain, desc, state, state_bytes, stream));
}
int m3_ctc_beam_ctx_reset(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, m3_stream stream) {
  return beam_reset(beam_call("ctc_beam_ctx_reset", BeamForm::Ctx, desc, state, state_bytes, stream));
}
int m3_ctc_beam_lm_reset(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, m3_stream stream) {
  return beam_reset(beam_call("ctc_beam_lm_reset", BeamForm::Lm, desc, state, state_bytes, stream));
}
int m3_ctc_beam_reset_slots(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n, m3_stream stream) {
  return beam_reset_slots(beam_call("ctc_beam_reset", BeamForm::Plain, desc, state, state_bytes, stream), slots, n);
}
int m3_ctc_beam_ctx_reset_slots(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                                m3_stream stream) {
  return beam_reset_slots(beam_call("ctc_beam_ctx_reset", BeamForm::Ctx, desc, state, state_bytes, stream), slots, n);
}
int m3_ctc_beam_lm_reset_slots(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                               m3_stream stream) {
  return beam_reset_slots(beam_call("ctc_beam_lm_reset", BeamForm::Lm, desc, state, state_bytes, stream), slots, n);
}
int m3_ctc_beam_advance(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const float* top_logp,
                        const int32_t* top_idx, int T_chunk, const int32_t* n_frames, m3_stream stream) {
  BeamCall c = beam_call("ctc_beam_advance", BeamForm::Plain, desc, state, state_bytes, stream);
  c.top_logp = top_logp; c.top_idx = top_idx; c.T_chunk = T_chunk; c.n_frames = n_frames;
  return beam_advance(c);
}
int m3_ctc_beam_ctx_advance(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const void* image, size_t image_bytes,
                            const int32_t* graph_of, const float* top_logp, const int32_t* top_idx, int T_chunk,
                            const int32_t* n_frames, m3_stream stream) {
  BeamCall c = beam_call("ctc_beam_ctx_advance", BeamForm::Ctx, desc, state, state_bytes, stream);
  c.image = image; c.image_bytes = image_bytes; c.graph_of = graph_of;
  c.top_logp = top_logp; c.top_idx = top_idx; c.T_chunk = T_chunk; c.n_frames = n_frames;
  return beam_advance(c);
}
int m3_ctc_beam_lm_advance(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const void* image, size_t image_bytes,
                           const int32_t* graph_of, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha,
                           double beta, const float* top_logp, const int32_t* top_idx, int T_chunk, const int32_t* n_frames,
                           m3_stream stream) {
  BeamCall c = beam_call("ctc_beam_lm_advance", BeamForm::Lm, desc, state, state_bytes, stream);
  c.image = image; c.image_bytes = image_bytes; c.graph_of = graph_of;
  c.lm_image = lm_image; c.lm_bytes = lm_bytes; c.lm_on = lm_on; c.alpha = alpha; c.beta = beta;
  c.top_logp = top_logp; c.top_idx = top_idx; c.T_chunk = T_chunk; c.n_frames = n_frames;
  return beam_advance(c);
}
int m3_ctc_beam_nbest(const m3_ctc_beam_desc* desc, const void* state, size_t state_bytes, int32_t* hyp_tokens,
                      int32_t* hyp_len, float* hyp_score, int32_t* n_hyps, m3_stream stream) {
  BeamCall c = beam_call("ctc_beam_nbest", BeamForm::Plain, desc, state, state_bytes, stream);
  c.hyp_tokens = hyp_tokens; c.hyp_len = hyp_len; c.hyp_score = hyp_score; c.n_hyps = n_hyps;
  return beam_nbest(c);
}
int m3_ctc_beam_ctx_nbest(const m3_ctc_beam_desc* desc, const void* state, size_t state_bytes, const void* image,
                          size_t image_bytes, const int32_t* graph_of, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score,
                          float* hyp_bonus, int32_t* n_hyps, m3_stream stream) {
  BeamCall c = beam_call("ctc_beam_ctx_nbest", BeamForm::Ctx, desc, state, state_bytes, stream);
  c.image = image; c.image_bytes = image_bytes; c.graph_of = graph_of;
  c.hyp_tokens = hyp_tokens; c.hyp_len = hyp_len; c.hyp_score = hyp_score; c.hyp_bonus = hyp_bonus; c.n_hyps = n_hyps;
  return beam_nbest(c);
}
int m3_ctc_beam_lm_nbest(const m3_ctc_beam_desc* desc, const void* state, size_t state_bytes, const void* image, size_t image_bytes,
                         const int32_t* graph_of, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha,
                         double beta, int use_eos, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, float* hyp_bonus,
                         float* hyp_lm, int32_t* n_hyps, m3_stream stream) {
  BeamCall c = beam_call("ctc_beam_lm_nbest", BeamForm::Lm, desc, state, state_bytes, stream);
  c.image = image; c.image_bytes = image_bytes; c.graph_of = graph_of;
  c.lm_image = lm_image; c.lm_bytes = lm_bytes; c.lm_on = lm_on; c.alpha = alpha; c.beta = beta; c.use_eos = use_eos;
  c.hyp_tokens = hyp_tokens; c.hyp_len = hyp_len; c.hyp_score = hyp_score; c.hyp_bonus = hyp_bonus; c.hyp_lm = hyp_lm;
  c.n_hyps = n_hyps;
  return beam_nbest(c);
}
size_t m3_ctc_align_workspace_size(const m3_ctc_align_desc* desc) { return ctc_align_workspace_size(desc); }
int m3_ctc_align_emit(const m3_ctc_align_desc* desc, const float* logits, int ldl, const int32_t* row0, const int32_t* n_frames,
                      const int32_t* tokens, const int32_t* tok0, float* emit, m3_stream stream) {
  return launch_ctc_align_emit(desc, logits, ldl, row0, n_frames, tokens, tok0, emit, (hipStream_t)stream);
}
int m3_ctc_align_path(const m3_ctc_align_desc* desc, const float* emit, const int32_t* n_frames, const int32_t* tokens,
                      const int32_t* tok0, void* workspace, size_t ws_bytes, float* score, int32_t* status, int32_t* state,
                      int32_t* tok_start, int32_t* tok_end, int32_t* tok_peak, float* tok_logp, m3_stream stream) {
  return launch_ctc_align_path(desc, emit, n_frames, tokens, tok0, workspace, ws_bytes, score, status, state, tok_start, tok_end,
                               tok_peak, tok_logp, (hipStream_t)stream);
}
int m3_ctc_context_validate(const void* image, size_t image_bytes, int V) { return ctc_context_validate(image, image_bytes, V); }
int m3_ctc_prefix_beam_search_ctx(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                  const void* image, size_t image_bytes, int graph, int32_t* hyp_tokens, int32_t* hyp_len,
                                  float* hyp_score, float* hyp_bonus, int32_t* hyp_state, int32_t* n_hyps) {
  return ctc_prefix_beam_search_ctx_host(top_logp, top_idx, T, k, beam, blank, image, image_bytes, graph, hyp_tokens, hyp_len,
                                         hyp_score, hyp_bonus, hyp_state, n_hyps);
}
int m3_ctc_lm_validate(const void* image, size_t image_bytes, int V) { return ctc_lm_validate(image, image_bytes, V); }
int m3_ctc_ngram_set_member(const void* image, size_t image_bytes, int j, const void** member, size_t* member_bytes, float* scale) {
  return ctc_lm_set_member(image, image_bytes, j, member, member_bytes, scale);
}
int m3_ctc_prefix_beam_search_lm(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                 const void* image, size_t image_bytes, int graph, const void* lm_image, size_t lm_bytes,
                                 double alpha, double beta, int use_eos, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score,
                                 float* hyp_bonus, int32_t* hyp_state, float* hyp_lm, int32_t* n_hyps) {
  return ctc_prefix_beam_search_lm_host(top_logp, top_idx, T, k, beam, blank, image, image_bytes, graph, lm_image, lm_bytes, alpha,
                                        beta, use_eos, hyp_tokens, hyp_len, hyp_score, hyp_bonus, hyp_state, hyp_lm, n_hyps);
}
int m3_wfst_validate(const void* image, size_t image_bytes, int V) { return wfst_validate(image, image_bytes, V); }
size_t m3_wfst_search_state_size(const m3_wfst_search_desc* desc) { return wfst_search_state_size(desc); }
int m3_wfst_search_reset(const m3_wfst_search_desc* desc, void* state, size_t state_bytes, const void* graph, size_t graph_bytes,
                         const int32_t* slots, int n, m3_stream stream) {
  return launch_wfst_search_reset(desc, state, state_bytes, graph, graph_bytes, slots, n, (hipStream_t)stream);
}
int m3_wfst_search_advance(const m3_wfst_search_desc* desc, void* state, size_t state_bytes, const void* graph, size_t graph_bytes,
                           const float* logp, int ld, int T_chunk, const int32_t* n_frames, m3_stream stream) {
  return launch_wfst_search_advance(desc, state, state_bytes, graph, graph_bytes, logp, ld, T_chunk, n_frames, (hipStream_t)stream);
}
int m3_wfst_search_result(const m3_wfst_search_desc* desc, const void* state, size_t state_bytes, const void* graph,
                          size_t graph_bytes, int final, int max_words, int32_t* words, int32_t* frames, int32_t* n_words,
                          float* cost, int32_t* flags, int32_t* status, m3_stream stream) {
  return launch_wfst_search_result(desc, state, state_bytes, graph, graph_bytes, final, max_words, words, frames, n_words, cost,
                                   flags, status, (hipStream_t)stream);
}
size_t m3_wfst_skip_state_size(const m3_wfst_skip_desc* desc) { return wfst_skip_state_size(desc); }
int m3_wfst_skip_reset(const m3_wfst_skip_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n, m3_stream stream) {
  return launch_wfst_skip_reset(desc, state, state_bytes, slots, n, (hipStream_t)stream);
}
int m3_wfst_skip_select(const m3_wfst_skip_desc* desc, void* state, size_t state_bytes, const float* logp, int ld, int T_chunk,
                        const int32_t* n_frames, float* out, int ld_out, int32_t* n_kept, m3_stream stream) {
  return launch_wfst_skip_select(desc, state, state_bytes, logp, ld, T_chunk, n_frames, out, ld_out, n_kept, (hipStream_t)stream);
}
int m3_wfst_skip_map_frames(const m3_wfst_skip_desc* desc, const void* state, size_t state_bytes, int32_t* frames, int ld_frames,
                            const int32_t* n_words, m3_stream stream) {
  return launch_wfst_skip_map_frames(desc, state, state_bytes, frames, ld_frames, n_words, (hipStream_t)stream);
}
int m3_wfst_skip_counts(const m3_wfst_skip_desc* desc, const void* state, size_t state_bytes, int32_t* seen, int32_t* kept,
                        m3_stream stream) {
  return launch_wfst_skip_counts(desc, state, state_bytes, seen, kept, (hipStream_t)stream);
}
size_t m3_ctc_greedy_stream_state_size(const m3_ctc_greedy_desc* desc) { return ctc_greedy_stream_state_size(desc); }
int m3_ctc_greedy_stream_reset(const m3_ctc_greedy_desc* desc, void* state, size_t state_bytes, m3_stream stream) {
  return launch_ctc_greedy_stream_reset(desc, state, state_bytes, (hipStream_t)stream);
}
int m3_ctc_greedy_stream_reset_slots(const m3_ctc_greedy_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                                     m3_stream stream) {
  M3_REQUIRE(n == 0 || slots != nullptr, "ctc_greedy_stream_reset_slots: null slot list");
  if (n == 0) return 0;
  return launch_ctc_greedy_stream_reset(desc, state, state_bytes, (hipStream_t)stream, slots, n);
}
int m3_ctc_greedy_stream_advance(const m3_ctc_greedy_desc* desc, void* state, size_t state_bytes, const float* logits,
                                 int T_chunk, int V, const int32_t* n_frames, int32_t* frame_ids, m3_stream stream) {
  return launch_ctc_greedy_stream_advance(desc, state, state_bytes, logits, T_chunk, V, n_frames, frame_ids, (hipStream_t)stream);
}
int m3_ctc_greedy_stream_tokens(const m3_ctc_greedy_desc* desc, const void* state, size_t state_bytes, int32_t* tokens,
                                int32_t* n_tokens, m3_stream stream) {
  return launch_ctc_greedy_stream_tokens(desc, state, state_bytes, tokens, n_tokens, (hipStream_t)stream);
}
size_t m3_ctc_endpoint_state_size(const m3_ctc_endpoint_desc* desc) { return ctc_endpoint_state_size(desc); }
int m3_ctc_endpoint_reset(const m3_ctc_endpoint_desc* desc, void* state, size_t state_bytes, m3_stream stream) {
  return launch_ctc_endpoint_reset(desc, state, state_bytes, (hipStream_t)stream);
}
int m3_ctc_endpoint_reset_slots(const m3_ctc_endpoint_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                                m3_stream stream) {
  M3_REQUIRE(n == 0 || slots != nullptr, "ctc_endpoint_reset_slots: null slot list");
  if (n == 0) return 0;
  return launch_ctc_endpoint_reset(desc, state, state_bytes, (hipStream_t)stream, slots, n);
}
int m3_ctc_endpoint_advance(const m3_ctc_endpoint_desc* desc, void* state, size_t state_bytes, const float* top_logp,
                            const int32_t* top_idx, int T_chunk, int k, const int32_t* n_frames, m3_stream stream) {
  return launch_ctc_endpoint_advance(desc, state, state_bytes, top_logp, top_idx, T_chunk, k, n_frames, (hipStream_t)stream);
}
int m3_ctc_endpoint_read(const m3_ctc_endpoint_desc* desc, const void* state, size_t state_bytes, int32_t* info, m3_stream stream) {
  return launch_ctc_endpoint_read(desc, state, state_bytes, info, (hipStream_t)stream);
}
int m3_cat_split_cache(const void* in_cache, const void* input, int B, int cache_dim, int input_dim, void* output,
                       void* out_cache, m3_stream stream) {
  return launch_cat_split_cache(in_cache, input, B, cache_dim, input_dim, output, out_cache, (hipStream_t)stream);
}
int m3_att_stream_softmax(const float* scores, const int32_t* decode_frame_num, const int32_t* mask_idx, int B, int N,
                          int ld, int cache_len, float scale, float* out, m3_stream stream) {
  return launch_att_stream_softmax(scores, decode_frame_num, mask_idx, B, N, ld, cache_len, scale, out, (hipStream_t)stream);
}
int m3_rel_positional_encoding(const float* x, const float* pe, int pe_len, const int32_t* frame_num, int max_offset,
                               float scale, int B, int T, int D, float* y, float* pos_emb, int32_t* frame_num_out,
                               m3_stream stream) {
  return launch_rel_positional_encoding(x, pe, pe_len, frame_num, max_offset, scale, B, T, D, y, pos_emb, frame_num_out,
                                        (hipStream_t)stream);
}
int m3_masked_fill(const float* x, const int32_t* len, int B, int C, int T, float fill, float* y, m3_stream stream) {
  return launch_masked_fill(x, len, B, C, T, fill, y, (hipStream_t)stream);
}
int m3_glu(const float* x, int outer, int C, int inner, float* y, m3_stream stream) {
  return launch_glu(x, outer, C, inner, y, (hipStream_t)stream);
}
int m3_mask_conv2d_sample(const int32_t* len_in, int B, int left_padding, int stride, int32_t* len_out,
                          m3_stream stream) {
  return launch_mask_conv2d_sample(len_in, B, left_padding, stride, len_out, (hipStream_t)stream);
}
int m3_scale(const float* x, float scale, float* y, size_t n, m3_stream stream) {
  return launch_scale(x, scale, y, n, (hipStream_t)stream);
}
int m3_unary(const float* x, float* y, size_t n, int act, m3_stream stream) {
  return launch_unary(x, y, n, act, (hipStream_t)stream);
}
int m3_binary(const float* a, const float* b, float* y, const int64_t* shape, const int64_t* strides_a,
              const int64_t* strides_b, int ndim, int op, m3_stream stream) {
  return launch_binary_bcast(a, b, y, shape, strides_a, strides_b, ndim, op, (hipStream_t)stream);
}
int m3_permute(const float* x, float* y, const int64_t* out_shape, const int64_t* in_strides, int ndim,
               m3_stream stream) {
  return launch_permute(x, y, out_shape, in_strides, ndim, (hipStream_t)stream);
}
int m3_concat_last(const float* a, int da, const float* b, int db, float* y, size_t rows, m3_stream stream) {
  return launch_concat_last(a, da, b, db, y, rows, (hipStream_t)stream);
}
int m3_softmax(const float* x, float* y, size_t rows, int n, m3_stream stream) {
  return launch_softmax_lastdim(x, y, rows, n, (hipStream_t)stream);
}
int m3_batched_matmul(const float* a, const float* b, float* c, int batch, int M, int N, int K, int64_t stride_a,
                      int64_t stride_b, int transpose_b, m3_stream stream) {
  return launch_bmm(a, b, c, batch, M, N, K, stride_a, stride_b, transpose_b, (hipStream_t)stream);
}
int m3_pad2d(const float* x, size_t outer, int H, int W, int pre_h, int post_h, int pre_w, int post_w, float* y, m3_stream stream) {
  M3_REQUIRE(x && y, "pad2d: null pointer");
  return launch_pad2d(x, outer, H, W, pre_h, post_h, pre_w, post_w, y, (hipStream_t)stream);
}
int m3_depthwise_conv1d(const float* x, const float* w, const float* bias, int B, int C, int T, int K, int pad,
                        float* y, m3_stream stream) {
  return launch_depthwise_conv1d_nct(x, w, bias, B, C, T, K, pad, y, (hipStream_t)stream);
}

static int fbank_options_ok(int num_mel_bins, float sample_rate, float low_freq, float high_freq) {
  M3_REQUIRE(num_mel_bins >= 1 && num_mel_bins <= 128, "fbank: num_mel_bins=%d outside [1, 128]", num_mel_bins);
  M3_REQUIRE(sample_rate == 16000.f, "fbank: sample_rate=%g (only 16000 Hz)", sample_rate);
  M3_REQUIRE(low_freq >= 0.f && low_freq < high_freq && high_freq <= 0.5f * sample_rate,
             "fbank: need 0 <= low_freq=%g < high_freq=%g <= %g", low_freq, high_freq, 0.5f * sample_rate);
  return 0;
}
size_t m3_fbank_tables_bytes(int num_mel_bins) {
  if (num_mel_bins < 1 || num_mel_bins > 128) {
    set_error("fbank: num_mel_bins=%d outside [1, 128]", num_mel_bins);
    return 0;
  }
  return fbank_tables_bytes();
}
int m3_fbank_tables_host(int num_mel_bins, float sample_rate, float low_freq, float high_freq, void* host_tables) {
  M3_REQUIRE(host_tables != nullptr, "fbank_tables_host: null pointer");
  if (int rc = fbank_options_ok(num_mel_bins, sample_rate, low_freq, high_freq)) return rc;
  return fbank_tables_build(num_mel_bins, sample_rate, low_freq, high_freq, host_tables);
}
int m3_fbank_tables_init(int num_mel_bins, float sample_rate, float low_freq, float high_freq, void* tables, m3_stream stream) {
  M3_REQUIRE(tables != nullptr && aligned16(tables), "fbank_tables_init: tables must be non-null and 16-byte aligned");
  if (int rc = fbank_options_ok(num_mel_bins, sample_rate, low_freq, high_freq)) return rc;
  std::vector<char> image(fbank_tables_bytes());
  if (int rc = fbank_tables_build(num_mel_bins, sample_rate, low_freq, high_freq, image.data())) return rc;
  M3_CHECK_HIP(hipMemcpyAsync(tables, image.data(), image.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
  M3_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));     // the host image dies with this call
  return 0;
}
int m3_fbank_num_frames(int n_samples) { return n_samples < 400 ? 0 : 1 + (n_samples - 400) / 160; }
int m3_fbank(const void* tables, const void* pcm, int pcm_is_int16, int ld_pcm, const int32_t* n_samples, int B, int T,
             int num_mel_bins, float* feat, int ld_feat, int32_t* feat_len_out, m3_stream stream) {
  M3_REQUIRE(tables && pcm && n_samples && feat && feat_len_out, "fbank: null pointer");
  M3_REQUIRE(num_mel_bins >= 1 && num_mel_bins <= 128, "fbank: num_mel_bins=%d outside [1, 128]", num_mel_bins);
  M3_REQUIRE(B >= 0 && T >= 1, "fbank: bad sizes B=%d T=%d", B, T);
  M3_REQUIRE(ld_feat >= num_mel_bins, "fbank: ld_feat=%d is shorter than a row of %d", ld_feat, num_mel_bins);
  const int per16 = pcm_is_int16 ? 8 : 4;
  M3_REQUIRE(ld_pcm >= 0 && ld_pcm % per16 == 0, "fbank: ld_pcm=%d must be a multiple of %d samples (16 bytes)", ld_pcm, per16);
  M3_REQUIRE(aligned16(tables) && aligned16(pcm), "fbank: tables / pcm must be 16-byte aligned");
  return launch_fbank(tables, pcm, pcm_is_int16, ld_pcm, n_samples, B, T, num_mel_bins, feat, ld_feat, feat_len_out,
                      (hipStream_t)stream);
}

int m3_deltas_tables_host(int order, int window, float* scales) {
  M3_REQUIRE(scales != nullptr, "deltas_tables_host: null pointer");
  return deltas_tables_build(order, window, scales);
}
int m3_add_deltas(const float* feat, int ld_feat, int64_t batch_stride_feat, int T_in, const int32_t* n_in, const int32_t* lead,
                  const int32_t* n_out, int B, int T_out, int bins, int order, int window, float* out, int ld_out,
                  int64_t batch_stride_out, int32_t* out_len, m3_stream stream) {
  if (int rc = deltas_options_ok(order, window)) return rc;
  M3_REQUIRE(B >= 0 && B <= 65535 && T_in >= 0 && T_out >= 0, "add_deltas: bad sizes B=%d T_in=%d T_out=%d", B, T_in, T_out);
  M3_REQUIRE(bins >= 1 && bins <= 256, "add_deltas: bins=%d outside [1, 256]", bins);
  if (B == 0 || T_out == 0) return 0;
  M3_REQUIRE(feat && n_in && n_out && out, "add_deltas: null pointer");
  M3_REQUIRE(ld_feat >= bins && batch_stride_feat >= 0, "add_deltas: ld_feat=%d is shorter than a row of %d, or a negative batch stride",
             ld_feat, bins);
  M3_REQUIRE(ld_out >= (order + 1) * bins && batch_stride_out >= 0,
             "add_deltas: ld_out=%d is shorter than a row of %d columns, or a negative batch stride", ld_out, (order + 1) * bins);
  // the in-place form writes beside the static columns it reads; any other overlap would read what it has written
  M3_REQUIRE(out != feat || (ld_out == ld_feat && batch_stride_out == batch_stride_feat && lead == nullptr),
             "add_deltas: out == feat is the in-place form: it needs equal strides and lead == nullptr");
  return launch_add_deltas(feat, ld_feat, batch_stride_feat, T_in, n_in, lead, n_out, B, T_out, bins, order, window, out, ld_out,
                           batch_stride_out, out_len, (hipStream_t)stream);
}

static int resample_rates_ok(const char* who, int rate_in, int rate_out) {
  M3_REQUIRE(rate_in >= 1000 && rate_in <= 384000, "%s: rate_in=%d outside [1000, 384000]", who, rate_in);
  M3_REQUIRE(rate_out >= 1000 && rate_out <= 384000, "%s: rate_out=%d outside [1000, 384000]", who, rate_out);
  return 0;
}
size_t m3_resample_tables_bytes(int rate_in, int rate_out) { return resample_tables_bytes(rate_in, rate_out); }
int m3_resample_tables_host(int rate_in, int rate_out, void* host_tables) {
  M3_REQUIRE(host_tables != nullptr, "resample_tables_host: null pointer");
  return resample_tables_build(rate_in, rate_out, host_tables);
}
int m3_resample_tables_init(int rate_in, int rate_out, void* tables, m3_stream stream) {
  M3_REQUIRE(tables != nullptr && aligned16(tables), "resample_tables_init: tables must be non-null and 16-byte aligned");
  const size_t bytes = resample_tables_bytes(rate_in, rate_out);
  if (bytes == 0) return -2;
  std::vector<char> image(bytes);
  if (int rc = resample_tables_build(rate_in, rate_out, image.data())) return rc;
  M3_CHECK_HIP(hipMemcpyAsync(tables, image.data(), image.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
  M3_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));     // the host image dies with this call
  return 0;
}
int64_t m3_resample_num_samples(int rate_in, int rate_out, int64_t n_in, int flush) {
  if (resample_rates_ok("resample_num_samples", rate_in, rate_out)) return -1;
  return resample_num_samples(rate_in, rate_out, n_in, flush);
}
int m3_resample_input_span(int rate_in, int rate_out, int64_t out0, int64_t n_out, int64_t* first_in, int64_t* end_in) {
  M3_REQUIRE(first_in && end_in, "resample_input_span: null pointer");
  if (int rc = resample_rates_ok("resample_input_span", rate_in, rate_out)) return rc;
  M3_REQUIRE(out0 >= 0, "resample_input_span: out0=%lld is negative", (long long)out0);
  long f = 0, e = 0;
  resample_input_span(rate_in, rate_out, out0, n_out, &f, &e);
  *first_in = f;
  *end_in = e;
  return 0;
}
int m3_resample(const void* tables, const void* pcm, int pcm_is_int16, int channels, int channel, int ld_pcm, const int64_t* in0,
                const int32_t* n_in, const int64_t* out0, const int32_t* n_out, int B, int N_out, float* out, int ld_out,
                m3_stream stream) {
  M3_REQUIRE(tables && pcm && in0 && n_in && out0 && n_out && out, "resample: null pointer");
  M3_REQUIRE(channels >= 1 && channels <= 8, "resample: channels=%d outside [1, 8]", channels);
  M3_REQUIRE(channel >= -1 && channel < channels, "resample: channel=%d outside [-1, %d)", channel, channels);
  M3_REQUIRE(B >= 0 && B <= 65535 && N_out >= 0, "resample: bad sizes B=%d N_out=%d", B, N_out);
  M3_REQUIRE(ld_out >= N_out, "resample: ld_out=%d is shorter than a row of %d", ld_out, N_out);
  const int per16 = pcm_is_int16 ? 8 : 4;
  M3_REQUIRE(ld_pcm >= 0 && ld_pcm % per16 == 0, "resample: ld_pcm=%d must be a multiple of %d samples (16 bytes)", ld_pcm, per16);
  M3_REQUIRE(aligned16(tables) && aligned16(pcm) && aligned16(out), "resample: tables / pcm / out must be 16-byte aligned");
  return launch_resample(tables, pcm, pcm_is_int16, channels, channel, ld_pcm, in0, n_in, out0, n_out, B, N_out, out, ld_out,
                         (hipStream_t)stream);
}

int m3_vad_log_energy(const void* pcm, int pcm_is_int16, int ld_pcm, const int32_t* n_samples, int B, int T, float* log_energy,
                      int ld_out, int32_t* len_out, m3_stream stream) {
  M3_REQUIRE(B >= 0 && T >= 0, "vad_log_energy: bad sizes B=%d T=%d", B, T);
  if (B == 0 || T == 0) return 0;
  M3_REQUIRE(pcm && n_samples && log_energy && len_out, "vad_log_energy: null pointer");
  M3_REQUIRE(ld_out >= T, "vad_log_energy: ld_out=%d is shorter than a row of %d", ld_out, T);
  const int per16 = pcm_is_int16 ? 8 : 4;
  M3_REQUIRE(ld_pcm >= 0 && ld_pcm % per16 == 0, "vad_log_energy: ld_pcm=%d must be a multiple of %d samples (16 bytes)", ld_pcm, per16);
  M3_REQUIRE(aligned16(pcm), "vad_log_energy: pcm must be 16-byte aligned");
  return launch_vad_log_energy(pcm, pcm_is_int16, ld_pcm, n_samples, B, T, log_energy, ld_out, len_out, (hipStream_t)stream);
}
int m3_vad_decide(const float* log_energy, int ld_e, const int32_t* lens, int B, int T, float energy_threshold,
                  float energy_mean_scale, int context, float proportion_threshold, uint8_t* flags, int ld_flags,
                  float* threshold_out, m3_stream stream) {
  if (int rc = vad_options_ok(energy_mean_scale, context, proportion_threshold)) return rc;
  M3_REQUIRE(energy_threshold == energy_threshold, "vad_decide: energy_threshold is not a number");
  M3_REQUIRE(B >= 0 && B <= 65535 && T >= 0, "vad_decide: bad sizes B=%d T=%d", B, T);
  if (B == 0 || T == 0) return 0;
  M3_REQUIRE(log_energy && lens && flags && threshold_out, "vad_decide: null pointer");
  M3_REQUIRE(ld_e >= T && ld_flags >= T, "vad_decide: ld_e=%d or ld_flags=%d is shorter than a row of %d", ld_e, ld_flags, T);
  return launch_vad_decide(log_energy, ld_e, lens, B, T, energy_threshold, energy_mean_scale, context, proportion_threshold, flags,
                           ld_flags, threshold_out, (hipStream_t)stream);
}
int m3_vad_segments(const uint8_t* flags, int ld_flags, const float* log_energy, int ld_e, const int32_t* lens, int B, int T,
                    int min_silence, int min_speech, int pad, int max_segment, int split_search, int32_t* segments,
                    int capacity, int32_t* n_segments, m3_stream stream) {
  if (int rc = segment_options_ok(min_silence, min_speech, pad, max_segment, split_search)) return rc;
  M3_REQUIRE(B >= 0 && T >= 0 && capacity >= 0, "vad_segments: bad sizes B=%d T=%d capacity=%d", B, T, capacity);
  if (B == 0 || T == 0) return 0;
  M3_REQUIRE(flags && log_energy && lens && n_segments && (segments || capacity == 0), "vad_segments: null pointer");
  M3_REQUIRE(ld_e >= T && ld_flags >= T, "vad_segments: ld_e=%d or ld_flags=%d is shorter than a row of %d", ld_e, ld_flags, T);
  return launch_vad_segments(flags, ld_flags, log_energy, ld_e, lens, B, T, min_silence, min_speech, pad, max_segment,
                             split_search, segments, capacity, n_segments, (hipStream_t)stream);
}
int m3_segment_gather(const float* src, int ld_src, int T_all, const int32_t* jobs, int B, int T_max, int cols, float* dst,
                      int ld_dst, int64_t batch_stride_dst, int32_t* len_out, m3_stream stream) {
  M3_REQUIRE(B >= 0 && B <= 65535 && T_max >= 0 && T_all >= 0, "segment_gather: bad sizes B=%d T_max=%d T_all=%d", B, T_max, T_all);
  M3_REQUIRE(cols >= 1, "segment_gather: cols=%d", cols);
  if (B == 0 || T_max == 0) return 0;
  M3_REQUIRE(jobs && dst && len_out && (src || T_all == 0), "segment_gather: null pointer");
  M3_REQUIRE(ld_src >= cols && ld_dst >= cols && batch_stride_dst >= 0,
             "segment_gather: ld_src=%d or ld_dst=%d is shorter than a row of %d columns, or a negative batch stride", ld_src, ld_dst, cols);
  return launch_segment_gather(src, ld_src, T_all, jobs, B, T_max, cols, dst, ld_dst, batch_stride_dst, len_out, (hipStream_t)stream);
}

}  // extern "C"
