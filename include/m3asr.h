/* m3asr.h -- C ABI of libm3asr_hip.so, the MI355X (gfx950) replacement for the reference's
 * TRTAPI++/plugin library (libtrtplugin++.so) on the 3M-ASR Conformer-MoE encoder hot path.
 *
 * Conventions (mirroring the reference's plugin ABI, fmoe_expert_plugin.h:45-73):
 *   - every tensor and every workspace is a CALLER-OWNED DEVICE pointer; weights are ordinary inputs,
 *     never copied or owned by an op (README.md:225); plain pointers and sizes only, no framework types;
 *   - `stream` is a hipStream_t passed as void*; ops only enqueue work on it (no host sync, no
 *     allocation -> every entry point is hipGraph-capturable), unlike the reference's FMoE enqueue
 *     which synchronises twice per layer (fmoe_expert_plugin.cpp:75-78,130).  One caveat: kernels that need more than
 *     64 KB of LDS opt in with hipFuncSetAttribute the FIRST time their entry point runs in a process (not a stream
 *     operation) -- call an entry point once outside a capture before capturing it; m3_engine_* does this at prepare;
 *   - return value: 0 = ok, non-zero = failure (reference: `int enqueue(...)`), message via
 *     m3_last_error() (reference only logs, common/common.h:26-38);
 *   - dtype codes 0/1/2 = the reference's HelperConfig.plugin_data_type (builder_helper.py:47-57).
 * Row layouts are row-major; "S" = B*T' tokens, D = idim, F = hidden_units, E = num_expert.
 *
 * Row strides.  Every `ld*` argument is the distance between two rows of its operand IN ELEMENTS of that operand.  Each entry
 * point states what it needs of them; anything else is rejected on the host, before a kernel is launched (non-zero status).
 * Two rules hold everywhere: a stride is at least the row width it belongs to (rows never overlap; not required of an operand
 * with a single row), and a row that a kernel reads or writes 16 bytes at a time needs a stride that keeps every row as
 * aligned as the first one: a multiple of 4 fp32 or 8 bf16 elements (4 for bf16 rows written 8 bytes at a time).  The base
 * pointer of every strided operand must be 16-byte aligned (checked with the strides).  Operands without a stride argument
 * are dense.  The whole-encoder engine builds its own operands inside the workspace and does not pass through these checks.
 */
#ifndef M3ASR_H_
#define M3ASR_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3ASR_ABI_VERSION 10

typedef void* m3_stream; /* hipStream_t */

enum m3_dtype { M3_F32 = 0, M3_F16 = 1, M3_I8 = 2, M3_I32 = 3, M3_BF16 = 4, M3_FP8 = 5 /* OCP e4m3 */,
                M3_MXFP4 = 6 /* bytes of an OCP MXFP4 tensor: e2m1 code pairs, or its e8m0 block scales */ };

/* activation / element-wise codes shared by several entry points */
enum m3_act { M3_ACT_NONE = 0, M3_ACT_RELU = 1, M3_ACT_SILU = 2, M3_ACT_GLU = 3, M3_ACT_SIGMOID = 4, M3_ACT_LOG = 5 };
enum m3_binop { M3_OP_SUM = 0, M3_OP_PROD = 1 };

/* ------------------------------------------------------------------------------------------------
 * Library / registry.   Replaces: initLibNvInferPlugins + getPluginRegistry (plugin/exports.map:18-27),
 * init_trt_plugin_plus (trt_plugin_plus.h:23) and PluginCreatorRegistry lookup (trt_plugin_plus.cpp:56-123).
 * ---------------------------------------------------------------------------------------------- */
int m3_abi_version(void);
const char* m3_last_error(void);
/* 1 if a creator for (name, version) is registered, else 0.  Names are the reference's plugin names. */
int m3_registry_lookup(const char* plugin_name, const char* plugin_version);
int m3_registry_count(void);
const char* m3_registry_name(int index);

/* ------------------------------------------------------------------------------------------------
 * Generic plugin objects.   Replaces IPluginCreator::createPlugin / IPluginV2DynamicExt
 * {getOutputDimensions, getWorkspaceSize, enqueue, serialize, clone, destroy} for the eight plugins of
 * the hot path (fmoe_expert_plugin.h:45-73 is the template all of them follow).
 * ---------------------------------------------------------------------------------------------- */
typedef struct m3_tensor { /* = nvinfer1::PluginTensorDesc + data pointer */
  void* data;
  int32_t dtype; /* enum m3_dtype */
  int32_t ndim;
  int64_t shape[8];
} m3_tensor;

enum m3_field_type { M3_FIELD_FLOAT32 = 1, M3_FIELD_INT32 = 5 }; /* values of nvinfer1::PluginFieldType */
typedef struct m3_field {                                          /* = nvinfer1::PluginField */
  const char* name;
  const void* data;
  int32_t type;
  int32_t length;
} m3_field;

typedef struct m3_plugin m3_plugin;

/* NULL on unknown plugin or bad/missing attributes (reference creators return nullptr,
 * fmoe_expert_plugin.cpp:356-359). */
m3_plugin* m3_plugin_create(const char* plugin_name, const char* plugin_version, const m3_field* fields,
                            int n_fields);
m3_plugin* m3_plugin_clone(const m3_plugin* plugin);
void m3_plugin_destroy(m3_plugin* plugin);
const char* m3_plugin_type(const m3_plugin* plugin);
int m3_plugin_num_outputs(const m3_plugin* plugin);
/* fills outputs[i].{dtype,ndim,shape} from the input descriptors (data pointers ignored) */
int m3_plugin_output_dims(const m3_plugin* plugin, const m3_tensor* inputs, int n_in, m3_tensor* outputs,
                          int n_out);
size_t m3_plugin_workspace_size(const m3_plugin* plugin, const m3_tensor* inputs, int n_in,
                                const m3_tensor* outputs, int n_out);
int m3_plugin_enqueue(m3_plugin* plugin, const m3_tensor* inputs, int n_in, m3_tensor* outputs, int n_out,
                      void* workspace, size_t workspace_bytes, m3_stream stream);
/* POD serialisation of the attributes (reference: serialize.hpp:36-52) */
size_t m3_plugin_serialization_size(const m3_plugin* plugin);
int m3_plugin_serialize(const m3_plugin* plugin, void* buffer, size_t bytes);
m3_plugin* m3_plugin_deserialize(const char* plugin_name, const char* plugin_version, const void* buffer,
                                 size_t bytes);

/* ------------------------------------------------------------------------------------------------
 * MoE hot path, direct entry points (what FMoEExpertPluginDynamic's enqueue is made of).
 * ---------------------------------------------------------------------------------------------- */
/* Replaces ComputeScatterMapping (fmoe_expert_kernel.h:26-27; fmoe_expert_kernel.cu:25-90).
 * gate_idx[S] int32 in [0,E) (or <0 = dropped row) -> mapping[S], acc_histogram[E+1], pos[S] (inverse
 * permutation, may be NULL).  Stable within an expert. */
int m3_moe_scatter_mapping(const int32_t* gate_idx, int S, int num_expert, int32_t* mapping,
                           int32_t* acc_histogram, int32_t* pos, m3_stream stream);
/* Replaces ComputeScatterMappingCopy (fmoe_expert_kernel.cu:92-128) = FastMoE local_scatter
 * (fmoe/functions.py:72):  out[mapping[s]] = x[s];  rows of row_bytes (multiple of 16). */
int m3_moe_local_scatter(const void* x, const int32_t* mapping, int S, int row_bytes, void* out,
                         m3_stream stream);
/* Replaces ComputeGatherrMappingCopy (fmoe_expert_kernel.cu:191-227) = FastMoE local_gather
 * (fmoe/functions.py:194):  out[s] = buf[mapping[s]] (0 for dropped rows). */
int m3_moe_local_gather(const void* buf, const int32_t* mapping, int S, int row_bytes, void* out,
                        m3_stream stream);
/* Hidden units per work-group of the grouped expert FFN: the engine's expert w_2 is stored slice-major
 * [E][F/slice][D][slice] (m3asr/plan.py); plugin-path weights keep the reference layout [E][D][F]. */
int m3_moe_expert_slice(void);
/* Workspace of m3_moe_expert_ffn / FMoEExpertPluginDynamic (reference layout: fmoe_expert_plugin.cpp:224-239). */
size_t m3_moe_expert_workspace_size(int S, int num_expert, int idim, int hidden_units);
/* Replaces compute_fmoe_expert (fmoe_expert_plugin.cpp:36-142): y[s] = SiLU(x[s] W1[g]^T + b1[g]) W2[g]^T + b2[g]
 * for g = gate_idx[s] >= 0, else 0.  x,y [S][D] f32; w1 [E][F][D], b1 [E][F], w2 [E][D][F], b2 [E][D]
 * (FMoELinear layout, fmoe/layers.py:34-38).  Optional fused epilogue (all may be NULL / 1.0):
 *   y[s] = resid[s] + alpha * gate_value[s] * y[s], then LayerNorm(ln_gamma, ln_beta, ln_eps). */
int m3_moe_expert_ffn(const float* x, const int32_t* gate_idx, const float* w1, const float* b1,
                      const float* w2, const float* b2, int S, int num_expert, int idim, int hidden_units,
                      const float* gate_value, const float* resid, float alpha, const float* ln_gamma,
                      const float* ln_beta, float ln_eps, float* y, void* workspace, size_t workspace_bytes,
                      m3_stream stream);
/* The same with w1 and w2 in fragment order (see m3_linear_wfrag below for the layout): w1 [E][F][D] packed per expert with N = F,
 * K = D, i.e. [E][F/16][D/16][4][16][4]; w2 packed from its slice-major form [E][F/slice][D][slice] with N = D, K = slice, i.e.
 * [E][F/slice][D/16][slice/16][4][16][4] -- the loads of one output tile are one contiguous run.  Both 16-byte aligned.  Same bits
 * as m3_moe_expert_ffn.  Exists for the one-launch fp32 form (S < 1024 rows); a shape that runs another form FAILS. */
int m3_moe_expert_ffn_wfrag(const float* x, const int32_t* gate_idx, const float* w1, const float* b1,
                            const float* w2, const float* b2, int S, int num_expert, int idim, int hidden_units,
                            const float* gate_value, const float* resid, float alpha, const float* ln_gamma,
                            const float* ln_beta, float ln_eps, float* y, void* workspace, size_t workspace_bytes,
                            m3_stream stream);
/* The same with bf16 expert weights (w1 / w2 point at bf16 [E][F][D] / [E][D][F]; biases, rows, epilogue fp32):
 * the half-precision mode the reference declares (`data_type` plugin field, fmoe_expert_plugin.cpp:331-354) but
 * asserts on (:264-266).  Rows and H are rounded to bf16 at the MFMA inputs, accumulation is fp32. */
int m3_moe_expert_ffn_bf16(const float* x, const int32_t* gate_idx, const void* w1, const float* b1,
                           const void* w2, const float* b2, int S, int num_expert, int idim, int hidden_units,
                           const float* gate_value, const float* resid, float alpha, const float* ln_gamma,
                           const float* ln_beta, float ln_eps, float* y, void* workspace, size_t workspace_bytes,
                           m3_stream stream);
/* fp8 expert weights (W8A16): w1 / w2 hold OCP e4m3 bytes, W[e][n][k] ~ scale[e][n] * q[e][n][k] with w1_scale [E][F],
 * w2_scale [E][D]; the weights are dequantised to bf16 at the MFMA input (exact), rows and H are rounded to bf16 as in
 * the bf16 form, accumulation fp32.  1.05 MB per touched expert at D=512, F=1024. */
int m3_moe_expert_ffn_fp8(const float* x, const int32_t* gate_idx, const void* w1, const float* w1_scale,
                          const float* b1, const void* w2, const float* w2_scale, const float* b2, int S, int num_expert,
                          int idim, int hidden_units, const float* gate_value, const float* resid, float alpha,
                          const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                          size_t workspace_bytes, m3_stream stream);
/* MXFP4 expert weights (W4A16; added under ABI 10): OCP e2m1 elements, two codes per byte with the even-k element in the low
 * nibble, and one e8m0 scale byte per 32 consecutive k (m3asr/plan.py quantize_mxfp4 is the definition).  w1 [E][F][idim/2],
 * w1_scale [E][F][idim/32], w2 [E][idim][F/2], w2_scale [E][idim][F/32], all bytes, 16-byte aligned.  idim % 128 == 0,
 * hidden_units % 64 == 0.  The weights are decoded to bf16 at the MFMA input (exact), rows and H are rounded to bf16 as in
 * the bf16 form, accumulation fp32.  0.53 MB per touched expert at D=512, F=1024.  _ldx: the same on rows of stride ldx
 * (a multiple of 4, >= idim). */
int m3_moe_expert_ffn_mxfp4(const float* x, const int32_t* gate_idx, const void* w1, const void* w1_scale,
                            const float* b1, const void* w2, const void* w2_scale, const float* b2, int S, int num_expert,
                            int idim, int hidden_units, const float* gate_value, const float* resid, float alpha,
                            const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                            size_t workspace_bytes, m3_stream stream);
int m3_moe_expert_ffn_mxfp4_ldx(const float* x, int ldx, const int32_t* gate_idx, const void* w1, const void* w1_scale,
                                const float* b1, const void* w2, const void* w2_scale, const float* b2, int S, int num_expert,
                                int idim, int hidden_units, const float* gate_value, const float* resid, float alpha,
                                const float* ln_gamma, const float* ln_beta, float ln_eps, float* y, void* workspace,
                                size_t workspace_bytes, m3_stream stream);
/* fp8 ARITHMETIC (A8W8; the path the reference's --int8 flag names, builder.py:39-49): e4m3 weights as above, the rows
 * quantised to e4m3 with a per-row dynamic scale (amax / 448) while they are loaded, H quantised with the static per-layer
 * scale h_scale (calibrated: amax of H x 1.25 / 448), products on v_mfma_f32_32x32x16_fp8_fp8, fp32 accumulation.  Taken
 * where the fused fp8 kernel applies (m3_moe_expert_ffn_fp8a8_active: idim 512, >= 4096 rows, >= 64 rows per expert);
 * shorter inputs are weight-streaming bound and run the weight-only form of m3_moe_expert_ffn_fp8 (identical signature
 * otherwise). */
int m3_moe_expert_ffn_fp8a8(const float* x, const int32_t* gate_idx, const void* w1, const float* w1_scale,
                            const float* b1, const void* w2, const float* w2_scale, const float* b2, float h_scale, int S,
                            int num_expert, int idim, int hidden_units, const float* gate_value, const float* resid,
                            float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps, float* y,
                            void* workspace, size_t workspace_bytes, m3_stream stream);
int m3_moe_expert_ffn_fp8a8_active(int S, int num_expert, int idim, int hidden_units);
/* Host only: the kernel the grouped expert FFN runs for this weight dtype (M3_F32 / M3_BF16 / M3_FP8 / M3_MXFP4, fp8_activations 0/1: fp8 only) and shape,
 * its launch count and the number of partial-result slabs; NULL for a shape the operator rejects.  No pointer is dereferenced. */
const char* m3_moe_expert_ffn_kernel(int weight_dtype, int fp8_activations, int S, int num_expert, int idim, int hidden_units,
                                     int32_t* launches, int32_t* slices);
/* ABI 9.  The same operator on rows that are ALREADY quantised the way it quantises them itself: xq [S][idim] e4m3, xq_scale [S]
 * (x = xq * xq_scale per row; what m3_quantize_rows_e4m3 and, inside the engine, the router kernel write).  Where the fused
 * kernel applies (m3_moe_expert_ffn_fp8a8_active) x is not read and may be NULL, and the result is bit-identical to
 * m3_moe_expert_ffn_fp8a8 on the fp32 rows; elsewhere the weight-only form runs on x.  Replaces nothing in the reference (its
 * --int8 path asserts, builder.py:39-49); it is the hand-over the whole-encoder engine uses between its router kernel and its
 * expert kernel, exposed so that it can be tested at the boundary. */
int m3_moe_expert_ffn_fp8a8_xq(const float* x, const void* xq, const float* xq_scale, const int32_t* gate_idx, const void* w1,
                               const float* w1_scale, const float* b1, const void* w2, const float* w2_scale, const float* b2,
                               float h_scale, int S, int num_expert, int idim, int hidden_units, const float* gate_value,
                               const float* resid, float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps,
                               float* y, void* workspace, size_t workspace_bytes, m3_stream stream);
/* rows -> OCP e4m3 with one dynamic scale per row: scale[s] = amax(x[s]) / 448 (1e-30 floor), xq = round-to-nearest-even,
 * saturating (x[s] / scale[s]).  idim must be 512 (one wave per row).  ldx: multiple of 4, >= idim; xq / scale are dense. */
int m3_quantize_rows_e4m3(const float* x, int ldx, int S, int idim, void* xq, float* scale, m3_stream stream);
/* The tail of the MoE layer on rows that are already in scattered (expert-sorted) order, e.g. rows that came back
 * from the expert-parallel all-to-all:  out[s] = LayerNorm( resid[s] + alpha * gate_value[s] * rows[mapping[s]] )
 * (rows with mapping < 0 contribute 0; gate_value / resid / ln_* may be NULL).  = local_gather
 * (fmoe/functions.py:194) + addProd + addScale + addAdd + norm_final (fmoe_transformer.py:145-166). */
int m3_moe_combine(const float* rows, const int32_t* mapping, const float* gate_value, const float* resid,
                   float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps, float* out, int S,
                   int idim, m3_stream stream);
/* The same, also writing the bf16 copy of `out` that engines with bf16 activation operands keep of the residual stream
 * (engine buffer "xb"; out_bf16 = [S][idim] bf16, may be NULL): lets the expert-parallel driver stand in for the
 * engine's own combine stage in the 16-bit modes. */
int m3_moe_combine_bf16(const float* rows, const int32_t* mapping, const float* gate_value, const float* resid,
                        float alpha, const float* ln_gamma, const float* ln_beta, float ln_eps, float* out,
                        void* out_bf16, int S, int idim, m3_stream stream);
/* Expert-parallel exchange without a host round trip (replaces the host logic of FastMoE's moe_prepare_forward /
 * MOEScatter / MOEGather, trainer_3m_fix/fmoe/functions.py:13-52,63-86,175-199, which reads the counts back to size its
 * all-to-all-v).  The wire buffer has a FIXED shape [world][1 + capacity][row_bytes]: chunk j = what this rank sends to
 * (after the equal-split all-to-all: received from) rank j = one header row with the e_loc row counts of the chunk
 * (int32: the count exchange rides in the payload) + up to `capacity` rows sorted by rank j's local expert id.
 *   m3_ep_send_map : from the local index step (gate_idx = GLOBAL expert id or -1, mapping, acc_histogram over
 *                    world * e_loc experts) -> map_send[s] = wire row of token s (-1: dropped) and the headers written
 *                    into `wire`; local_scatter(x, map_send) then fills the payload, and the reply comes back at the same
 *                    row.  capacity >= S (a rank may send everything to one peer).
 *   m3_ep_recv_gate: from the headers of the received chunks -> gate_recv[world * (1 + capacity)] = local expert id of
 *                    every received wire row (-1: header / unused), the gate input of m3_moe_expert_ffn. */
int m3_ep_send_map(const int32_t* gate_idx, const int32_t* mapping, const int32_t* acc_histogram, int S, int world, int e_loc,
                   int capacity, int32_t* map_send, void* wire, int row_bytes, m3_stream stream);
int m3_ep_recv_gate(const void* wire, int world, int e_loc, int capacity, int row_bytes, int32_t* gate_recv, m3_stream stream);
/* Router of the MoE feed-forward (positionwise_feed_forward.py:169-180,225 + norm_ff, fmoe_transformer.py:138-141):
 * logits[S][num_expert] = cat([embed (S, embed_dim), LayerNorm(x) (S, idim)]) . w^T (+ bias), w [num_expert][embed_dim + idim]
 * fp32 row-major; xn (may be NULL) receives LayerNorm(x), the expert FFN's input.  num_expert <= 64, dims multiples of 64.
 * Strides: ld_embed >= embed_dim, ldx >= idim, ld_xn >= idim, each a multiple of 4 (16-byte row accesses); ld_logits >=
 * num_expert, any value (the logits are stored element by element). */
int m3_moe_router(const float* embed, int ld_embed, int embed_dim, const float* x, int ldx, int idim, const float* w,
                  const float* bias, const float* ln_gamma, const float* ln_beta, float ln_eps, float* xn, int ld_xn,
                  float* logits, int ld_logits, int S, int num_expert, m3_stream stream);
/* Replaces ComputeSoftmaxAndTop1 (softmax_topk_kernel.cu:88-120): logits [S][ld] -> idx[S], value[S];
 * frames t >= len[b] (t = s % rows_per_batch, b = s / rows_per_batch) get idx -1 / value 0; len may be NULL.
 * ld >= width, any value (element loads); idx / value are dense. */
int m3_softmax_top1(const float* logits, int ld, const int32_t* len, int rows_per_batch, int S, int width,
                    int32_t* idx, float* value, m3_stream stream);
/* ABI 10.  The routing launches the whole-encoder engine is built from, exposed so that they can be tested at the boundary
 * (they replace nothing more in the reference than the operators they fuse).  All three leave the same five results:
 * gate_idx[S] / gate_value[S] as m3_softmax_top1 (frames t >= row_len[b] get -1 / 0; row_len may be NULL), and mapping[S],
 * acc_histogram[num_expert + 1], pos (may be NULL; entries at and beyond acc_histogram[num_expert] are not written) as
 * m3_moe_scatter_mapping on that gate_idx.
 *   m3_moe_gate_index: SoftmaxTopK + ScatterMapping in one single-work-group launch.  logits [S][num_expert] dense,
 *                      16-byte aligned; num_expert 8 / 16 / 32 / 64, S >= 1. */
int m3_moe_gate_index(const float* logits, const int32_t* row_len, int rows_per_batch, int S, int num_expert,
                      int32_t* gate_idx, float* gate_value, int32_t* mapping, int32_t* acc_histogram, int32_t* pos,
                      m3_stream stream);
/*   m3_moe_route: the x half of the router product with the layer's LayerNorm folded into the weights,
 *                 logits[s][e] = (x[s] . wx[e] - mean_s * wsum[e]) * rstd_s + bias[e] + eall[s][e],
 *                 (wx [num_expert][idim] = w * gamma, wsum[e] = sum_k wx[e][k], bias = w . beta (+ router bias), may be NULL;
 *                 eall [S][ld_e] = the embed half, may be NULL), then SoftmaxTopK + ScatterMapping, in one single-work-group
 *                 launch.  1 <= S <= 256, num_expert 16 / 32 / 64, idim a multiple of 16, ldx >= idim a multiple of 4,
 *                 ld_e >= num_expert; x / wx 16-byte aligned. */
int m3_moe_route(const float* x, int ldx, int idim, const float* wx, const float* wsum, const float* bias, const float* eall,
                 int ld_e, float ln_eps, const int32_t* row_len, int rows_per_batch, int S, int num_expert, int32_t* gate_idx,
                 float* gate_value, int32_t* mapping, int32_t* acc_histogram, int32_t* pos, m3_stream stream);
/*   m3_moe_route_expert_ffn: SoftmaxTopK + ScatterMapping + the grouped fp32 expert FFN (+ b2) in one launch, then the
 *                 combine on rows that stayed at their original index:
 *                   y[s] = LayerNorm( resid[s] + alpha * gate_value[s] * (SiLU(xn[s] W1[g]^T + b1[g]) W2[g]^T + b2[g]) ),  g = gate_idx[s],
 *                 rows with gate_idx < 0 contribute 0.  xn = x, or LayerNorm(x; norm_gamma, norm_beta, norm_eps) applied while
 *                 the rows are gathered when norm_gamma != NULL.  use_gate_value = 0: the factor gate_value[s] is left out (the
 *                 tap is written all the same).  resid / ln_gamma / ln_beta may be NULL.  Weights as m3_moe_expert_ffn;
 *                 w2_sliced = 1: w2 is slice-major [E][F / slice][D][slice] (m3_moe_expert_slice); w2_sliced = 2: w1 AND w2 are
 *                 in fragment order, as m3_moe_expert_ffn_wfrag takes them (same bits).  1 <= S <= 256, num_expert
 *                 8 / 16 / 32 / 64, idim a multiple of 16 (<= 2048; with S > 64 the row tile must fit the LDS), hidden_units a
 *                 multiple of the slice, ldx >= idim a multiple of 4; x / logits 16-byte aligned.  workspace: the partial
 *                 results, m3_moe_route_expert_workspace_size bytes (0 for a shape the operator does not take). */
size_t m3_moe_route_expert_workspace_size(int S, int num_expert, int idim, int hidden_units);
int m3_moe_route_expert_ffn(const float* x, int ldx, const float* logits, const int32_t* row_len, int rows_per_batch,
                            const float* w1, const float* b1, const float* w2, int w2_sliced, const float* b2, int S,
                            int num_expert, int idim, int hidden_units, const float* norm_gamma, const float* norm_beta,
                            float norm_eps, int use_gate_value, const float* resid, float alpha, const float* ln_gamma,
                            const float* ln_beta, float ln_eps, int32_t* gate_idx, float* gate_value, int32_t* mapping,
                            int32_t* acc_histogram, int32_t* pos, float* y, void* workspace, size_t workspace_bytes,
                            m3_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Dense building blocks (TensorRT-native layers of the reference + the small plugins).
 * ---------------------------------------------------------------------------------------------- */
/* Linear / point-wise conv with fused prologue+epilogue.  Replaces addLinear_ (torch_network_helper.py:573-605),
 * addConv1d k=1 (:199-225), LayerNorm plugin (layer_norm_plugin.cpp:78-113), masked_fill, GLU, SiLU/ReLU,
 * addScale + addAdd.   y[M][ldy] = resid + alpha * mask_out( act( LN(mask_in(a))[M][K] . w[N][K]^T + bias ) ).
 * a2 != NULL: A = cat([a (K1 cols), a2 (K-K1 cols)], -1) (router input, positionwise_feed_forward.py:225).
 * act = M3_ACT_GLU halves the output width (columns n and n+N/2 are paired, torch GLU dim=-1): n_out = N / 2, else N.
 * Strides (M > 1):
 *   lda  >= k1 (K without a2), multiple of 4 (fp32 a) or 8 (bf16 a);   lda2 >= K - k1, multiple of 4;
 *   ldy  >= n_out; any value for an fp32 y (the tiled kernels store 16 bytes at a time when ldy and ldr are multiples of 4
 *        and element by element otherwise: same values either way), a multiple of 4 for a bf16 y;
 *   ldr  >= n_out, any value; y == resid (in-place update) needs ldr == ldy;
 *   ld_copy >= n_out, multiple of 4.
 * w, bias, the LayerNorm vectors, y_copy_stats and ln_stats are dense. */
typedef struct m3_linear_desc {
  const float* a; int32_t lda;
  const float* a2; int32_t lda2; int32_t k1;
  const void* w;   /* [N][K] row-major; fp32, or bf16 when weight_dtype = M3_BF16 */
  const float* bias;
  float* y; int32_t ldy;
  int32_t M, N, K;
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  /* folded LayerNorm (affine pre-multiplied into w / bias by the plan packer): the kernel normalises its
   * OUTPUT, y = rstd*(a.w^T - mean*ln_wsum) + bias; ln_wbeta = w.beta, needed only together with mask_in */
  const float* ln_wsum; const float* ln_wbeta;
  const int32_t* len; int32_t rows_per_batch; int32_t mask_in; int32_t mask_out;
  int32_t act; float alpha;
  const float* resid; int32_t ldr;
  /* M3_F32 (exact fp32 MFMA) or M3_BF16: weights stored bf16, A rounded to bf16 at the MFMA input,
   * fp32 accumulate and fp32 epilogue (the reference's plugin_data_type = 1, builder_helper.py:47-57; bf16
   * replaces fp16 on CDNA4).  bf16 supports plain A (no a2) and the folded LayerNorm only; K % 32 == 0. */
  int32_t weight_dtype;
  /* bf16 activation operands (16-bit modes, long batches; what the engine does between the GEMMs of a block):
   *   a_dtype = M3_BF16: `a` points at bf16 rows (lda in elements, % 8 == 0);  y_dtype = M3_BF16: `y` receives bf16;
   *   y_copy_bf16: an additional bf16 copy of the fp32 result (ld_copy in elements), e.g. of the residual stream;
   *   y_copy_stats: with it, per row and per 128-column tile the (sum, sum of squares) of the bf16 values stored
   *     ([M][N/128][2] floats) -- the row statistics a folded-LayerNorm GEMM needs when its bf16 operand goes to LDS
   *     without passing through registers (LDS-DMA kernel); ln_stats / ln_stat_parts: such statistics of `a` (their parts
   *     are summed), required with ln_wsum when a_dtype = M3_BF16 and the LDS-DMA kernel is to be used.  Only the LDS-DMA
   *     kernel (M >= 4096 rows, bf16 A, K % 64 == 0) reads or writes them: a call that passes either and lands on another
   *     kernel FAILS (non-zero status) rather than leaving stale statistics behind.
   * All zero / NULL = fp32 activations as before. */
  int32_t a_dtype, y_dtype;
  void* y_copy_bf16; int32_t ld_copy;
  float* y_copy_stats;
  const float* ln_stats; int32_t ln_stat_parts;
} m3_linear_desc;
int m3_linear(const m3_linear_desc* desc, m3_stream stream);
/* The same with a caller-owned workspace: deep-K problems with few output tiles (K >= 4096, e.g. the subsampling Linear of
 * a single utterance) run as a split-K tiled kernel + fixed-order reduce when m3_linear_workspace_size(desc) > 0 bytes
 * are provided; otherwise identical to m3_linear. */
size_t m3_linear_workspace_size(const m3_linear_desc* desc);
/* Host only: name of the device kernel m3_linear (with_workspace = 0) or m3_linear_ws given its workspace (1) runs for desc
 * (sizes, strides, dtypes and modes are read, no pointer is dereferenced).  NULL for every descriptor m3_linear rejects, whether
 * the descriptor itself is malformed or no kernel of the family takes the problem (e.g. a bf16 `a` below the tiled kernel's row
 * count, y_copy_stats below the LDS-DMA kernel's): m3_last_error() then holds the reason m3_linear would give. */
const char* m3_linear_kernel(const m3_linear_desc* desc, int with_workspace);
int m3_linear_ws(const m3_linear_desc* desc, void* workspace, size_t workspace_bytes, m3_stream stream);
/* Fragment order: a constant fp32 weight matrix W[N][K] (N % 16 == 0, K % 16 == 0) stored in the order the skinny fp32 kernel's
 * v_mfma_f32_16x16x4_f32 fragments consume it,
 *     Wf[N/16][K/16][4 (kq)][16 (col)][4]   with   Wf[nt][s][kq][col][j] = W[16*nt + col][16*s + 4*kq + j],
 * so that lane l = 16*kq + col of a wave reads bytes [16*l, 16*l + 16) of the 1 KB that belongs to (column tile nt, K-step s):
 * one wave load instruction is one contiguous KB in lane order, not 16 pieces of 64 B from 16 rows.  Every lane receives the 16
 * bytes it receives from the row-major matrix, so results are bit for bit the same.
 * m3_pack_wfrag_host: host only, w[N][K] -> wf (N*K floats, must not overlap w).
 * m3_linear_wfrag: m3_linear with desc->w in fragment order (16-byte aligned).  Taken where desc plans as the skinny fp32 kernel
 * with plain A (no a2), fp32 weights, N (M3_ACT_GLU: N / 2) and K multiples of 16; every other descriptor FAILS with the reason
 * in m3_last_error().  m3_linear_wfrag_kernel: host only, the kernel's name or NULL with that reason.
 * m3_linear_pair_wfrag: m3_linear_pair with both w in fragment order. */
int m3_pack_wfrag_host(const float* w, int N, int K, float* wf);
int m3_linear_wfrag(const m3_linear_desc* desc, m3_stream stream);
const char* m3_linear_wfrag_kernel(const m3_linear_desc* desc);
int m3_linear_pair_wfrag(const m3_linear_desc* a, const m3_linear_desc* b, m3_stream stream);

/* LayerNormPluginDynamic (layer_norm_plugin.cpp:78-113) -- with eps, as PyTorch. */
int m3_layer_norm(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int dim,
                  m3_stream stream);
/* Fused rel-pos attention core; replaces attention.py:347-384 + :199-236 (shuffles, 3 batched matmuls,
 * AttMaskedSoftmaxPluginDynamic).  qkv [B*T][ldq] = (q|k|v), p [T][ldp], pos_u/pos_v [H][dk], out [B*T][ldo].
 * Strides (D = H * dk): ldq >= 3 D and ldp >= D, multiples of 4 (16-byte row loads); ldo >= D, any value (element stores).
 * The same holds for m3_relpos_attention_chunk. */
int m3_relpos_attention(const float* qkv, int ldq, const float* p, int ldp, const float* pos_u,
                        const float* pos_v, const int32_t* len, int B, int T, int H, int dk, float scale,
                        float* out, int ldo, m3_stream stream);
/* The same operator on bf16 rows (16-bit modes of long batches): qkv and out are bf16 ([B*T][ldq] / [B*T][ldo], strides in
 * elements), p / pos_u / pos_v stay fp32; bf16 MFMA, fp32 softmax; T <= 128 keys, dk 64 or 128.
 * Strides: ldq >= 3 D, multiple of 8; ldp >= D, multiple of 4; ldo >= D, multiple of 4 (8-byte row stores). */
int m3_relpos_attention_bf16(const void* qkv, int ldq, const float* p, int ldp, const float* pos_u, const float* pos_v,
                             const int32_t* len, int B, int T, int H, int dk, float scale, int chunk, int left_chunks,
                             void* out, int ldo, m3_stream stream);
/* The fp32 core with the static chunk mask of the streaming encoders (utils/mask.py:42-75,127-134): chunk > 0: query i
 * sees keys [max((i / chunk - left_chunks) chunk, 0), min((i / chunk + 1) chunk, T)) (all left chunks when left_chunks < 0)
 * and < len[b]; rows with no visible key give zeros.  chunk <= 0: identical to m3_relpos_attention. */
int m3_relpos_attention_chunk(const float* qkv, int ldq, const float* p, int ldp, const float* pos_u, const float* pos_v,
                              const int32_t* len, int B, int T, int H, int dk, float scale, int chunk, int left_chunks,
                              float* out, int ldo, m3_stream stream);
/* Depthwise conv (k odd, pad (k-1)/2) + LayerNorm (gamma NULL = none) + SiLU on channel-last rows;
 * replaces convolution.py:134-152.  w_kc [K][D] = depthwise weight (D,1,K) transposed. */
int m3_dwconv_ln_silu(const float* z, const float* w_kc, const float* bias, const float* gamma,
                      const float* beta, float eps, int B, int T, int D, int K, float* out, m3_stream stream);
/* The same with the GLU (glu_kernel.cu:26-44) of the convolution module applied where the conv loads its input: vg [B*T][ldz]
 * holds pointwise_conv1's raw output, value columns [0, D) | gate columns [D, 2 D) (bias added), and every tap is
 * value * sigmoid(gate) -- bit for bit what m3_linear (act = M3_ACT_GLU) followed by m3_dwconv_ln_silu gives (the engine's
 * short fp32 inputs: the GEMM in front then is the plain form, M3_GLU_DEFER).  K odd, <= 15; 256 <= D <= 1024, D % 4 == 0;
 * ldz >= 2 D, a multiple of 4; vg 16-byte aligned.  out [B*T][D] dense. */
int m3_dwconv_glu_ln_silu(const float* vg, int ldz, const float* w_kc, const float* bias, const float* gamma,
                          const float* beta, float eps, int B, int T, int D, int K, float* out, m3_stream stream);
/* The two stateful launches of chunk-by-chunk decoding (m3_engine_forward_chunk[_slots] is built from them) and the dense causal
 * conv, exposed so that they can be tested at the boundary (additions only; tests/test_stream_kernels_gpu.py).
 *
 * m3_relpos_attention_stream: the attention core on the C frames of the current chunk under the static chunk mask.  qkv
 * [B*C][ldq] = (q|k|v) of the chunk, rows at and past chunk_len[b] hold finite values; hist [B][cap][2 D] = K | V rows of the
 * frames so far, a ring indexed by (absolute frame) % cap, which this launch also appends the chunk's C rows to (read only by
 * later chunks); p [p_rows][ldp] indexed by the key's absolute frame; chunk_len [B] valid frames of the chunk per utterance
 * (device int32); out [B*C][ldo].  Chunk number n = the device-side counter: keys [max((n - left_chunks) C, 0), n C + chunk_len[b])
 * (all frames so far when left_chunks < 0), so the rows equal those m3_relpos_attention_chunk(chunk = C) gives on the whole
 * utterance, bit for bit.
 *   slot_max_chunks < 0: lockstep, `step` is ONE device int32 shared by the batch.  The caller guarantees
 *                        (*step + 1) * C <= p_rows: the counter lives on the device, the entry cannot check it.
 *   slot_max_chunks >= 0: slot mode, `step` is int32 [B], one counter per utterance slot.  A slot with chunk_len[b] <= 0,
 *                        step[b] < 0 or step[b] >= slot_max_chunks is not live: zero context rows, its history untouched.
 *                        slot_max_chunks * C <= p_rows is checked.
 * Strides: ldq >= 3 D and ldp >= D, multiples of 4; ldo >= D, any value.  cap >= C and cap >= (left_chunks + 1) * C.
 * dk 16 / 32 / 64 / 128.  The caller advances the counter(s) between launches. */
int m3_relpos_attention_stream(const float* qkv, int ldq, float* hist, int cap, const float* p, int ldp, int p_rows, const float* pos_u,
                               const float* pos_v, const int32_t* chunk_len, const int32_t* step, int B, int C, int H, int dk,
                               float scale, int left_chunks, int slot_max_chunks, float* out, int ldo, m3_stream stream);
/* m3_dwconv_ln_silu_stream: causal depthwise conv (lorder K - 1, K >= 2, no taps to the right) + LayerNorm (gamma / beta NULL =
 * none) + SiLU on the T frames of the current chunk, z / out [B*T][D] fp32.  cache_pair [2][B][K-1][D]: half (counter & 1) holds
 * the K - 1 frames left of the chunk and is only read; the other half receives the last K - 1 frames of
 * [that half | z[b][0 : chunk_len[b])] (chunk_len = 0: a copy).  step / chunk_len / slot_max_chunks as above (slot mode needs
 * slot_max_chunks > 0; a slot that is not live leaves both halves of its pair alone).  D a multiple of 4, <= 4096. */
int m3_dwconv_ln_silu_stream(const float* z, const float* w_kc, const float* bias, const float* gamma, const float* beta, float eps, int B,
                             int T, int D, int K, float* cache_pair, const int32_t* step, const int32_t* chunk_len, int slot_max_chunks,
                             float* out, m3_stream stream);
/* m3_dwconv_ln_silu_causal: the same conv on whole utterances, dense padded rows z / out [B*T][D]; every frame left of frame 0
 * is the row left_fill [D] (convolution.py:43-49,118-123: what pointwise_conv1 + GLU make of the module's zero padding). */
int m3_dwconv_ln_silu_causal(const float* z, const float* w_kc, const float* bias, const float* gamma, const float* beta, float eps,
                             const float* left_fill, int B, int T, int D, int K, float* out, m3_stream stream);
/* Conv2dSubsampling4 (subsampling.py:103-145) on channel-last data: conv1 (1->C, 3x3, s2) + ReLU. */
int m3_subsample_conv1(const float* feat, const float* w9c, const float* bias, int B, int T, int idim, int C,
                       float* out, m3_stream stream);
/* the same with global CMVN folded into the input read (mean / istd [idim], may be NULL) */
int m3_subsample_conv1_cmvn(const float* feat, const float* w9c, const float* bias, const float* cmvn_mean,
                            const float* cmvn_istd, int B, int T, int idim, int C, float* out, m3_stream stream);
/* The plain operators behind network_helper.addConv2d (torch_network_helper.py:227-251; nn.Conv2d 3x3 / stride 2 / no
 * padding, channel-last data): act = M3_ACT_NONE gives the convolution alone, M3_ACT_RELU the fused form above. */
int m3_conv2d_3x3s2_first(const float* feat, const float* w9c, const float* bias, int B, int T, int idim, int C, int act,
                          float* out, m3_stream stream);
int m3_conv2d_3x3s2(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C, int act, float* out,
                    m3_stream stream);
/* second conv (C->C, 3x3, s2) + ReLU as implicit GEMM: in (B,T1,F1,C) -> out (B,T2,F2,C); w [C][3][3][C]. */
int m3_subsample_conv2(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C,
                       float* out, m3_stream stream);
/* m3_conv2d_3x3s2 with a caller-owned workspace: deep, few-tile problems (C a multiple of 64, 9 C >= 4096, at most 160 output
 * tiles of 64 x 64) run as the implicit-conv split-K kernel + fixed-order reduce when m3_conv2d_3x3s2_workspace_size(...) > 0
 * bytes are provided; otherwise identical to m3_conv2d_3x3s2 (the size query answers 0 for such a problem). */
size_t m3_conv2d_3x3s2_workspace_size(int B, int T1, int F1, int C, int act);
int m3_conv2d_3x3s2_ws(const float* in, const float* w, const float* bias, int B, int T1, int F1, int C, int act, float* out,
                       void* workspace, size_t workspace_bytes, m3_stream stream);

/* The paired launches of the B = 1 fp32 engine (two INDEPENDENT problems of one operator in one launch: a stage of the embed
 * encoder next to a stage of the main encoder's prefix), exposed so that they can be tested at the boundary (additions only;
 * tests/test_pair_kernels_gpu.py).  Each entry checks both problems as the single entry of the operator does, requires that the
 * two outputs do not overlap, and makes ONE launcher call; each half of the result is what the single entry gives on the same
 * operands, bit for bit.  A pair the kernels have no common instantiation for returns a non-zero status with the reason in
 * m3_last_error() and launches nothing.
 *
 * m3_linear_pair: two m3_linear problems that both plan as the skinny fp32 kernel with 16-row tiles (M <= 128, or few enough
 * tiles), 4 or 8 waves (K < 2048) and one load group per wave (K <= 512, or K = 1024), plain `a`, no affine LayerNorm, and that
 * agree in the wave count (K < 1024 / K >= 1024), in GLU or not and in folded LayerNorm or not.  M, N, K, strides and every
 * other epilogue field may differ.
 * m3_linear_ws_pair: two m3_linear_ws problems that both plan as split-K with their workspaces (bytes_x >=
 * m3_linear_workspace_size(x) > 0; the workspaces must not overlap).  which: 1 = the GEMM launch, 2 = the reduce launch,
 * 3 = both.
 * m3_linear_pair_kernel: host only; the label of the kernel m3_linear_pair (with_workspace = 0) or m3_linear_ws_pair given both
 * workspaces (1) runs, NULL with the reason in m3_last_error() for a pair they refuse. */
int m3_linear_pair(const m3_linear_desc* a, const m3_linear_desc* b, m3_stream stream);
int m3_linear_ws_pair(const m3_linear_desc* a, void* workspace_a, size_t bytes_a, const m3_linear_desc* b, void* workspace_b,
                      size_t bytes_b, int which, m3_stream stream);
const char* m3_linear_pair_kernel(const m3_linear_desc* a, const m3_linear_desc* b, int with_workspace);
/* m3_conv2d_3x3s2_ws_pair: two m3_conv2d_3x3s2_ws problems that both run as split-K (which: as above). */
typedef struct m3_conv2d_desc {
  const float* in; const float* w; const float* bias;
  int32_t B, T1, F1, C, act;
  float* out;
} m3_conv2d_desc;
int m3_conv2d_3x3s2_ws_pair(const m3_conv2d_desc* a, void* workspace_a, size_t bytes_a, const m3_conv2d_desc* b, void* workspace_b,
                            size_t bytes_b, int which, m3_stream stream);
/* m3_relpos_attention_pair: two m3_relpos_attention_chunk problems, each with dk 64 or 128 (the four combinations). */
typedef struct m3_attention_desc {
  const float* qkv; int32_t ldq;
  const float* p; int32_t ldp;
  const float* pos_u; const float* pos_v;
  const int32_t* len;
  int32_t B, T, H, dk;
  float scale;
  int32_t chunk, left_chunks;
  float* out; int32_t ldo;
} m3_attention_desc;
int m3_relpos_attention_pair(const m3_attention_desc* a, const m3_attention_desc* b, m3_stream stream);
/* m3_dwconv_ln_silu_pair: two depthwise conv + LayerNorm + SiLU problems with the same D, K and causality.  ldz = 0: z is the
 * dense [B*T][D] input of m3_dwconv_ln_silu (left_fill NULL) or m3_dwconv_ln_silu_causal (left_fill [D]); ldz > 0: z is the
 * value | gate rows of m3_dwconv_glu_ln_silu (both problems then), and with gate_sigmoided != 0 its gate columns hold
 * sigmoid(gate) already (every tap is value * gate'; no single entry has this form).  gamma / beta NULL: no LayerNorm. */
typedef struct m3_dwconv_desc {
  const float* z; int32_t ldz; int32_t gate_sigmoided;
  const float* w_kc; const float* bias; const float* gamma; const float* beta; float eps;
  const float* left_fill;
  int32_t B, T, D, K;
  float* out;
} m3_dwconv_desc;
int m3_dwconv_ln_silu_pair(const m3_dwconv_desc* a, const m3_dwconv_desc* b, m3_stream stream);
/* m3_subsample_conv1_pair: two first convs (m3_conv2d_3x3s2_first / m3_subsample_conv1_cmvn) on inputs of the same B, T and
 * idim; act = M3_ACT_NONE or M3_ACT_RELU, cmvn_mean / cmvn_istd NULL or both given.  feat_len / lens_out (first problem only,
 * NULL or both given): the launch also writes lens_out[b] = ((feat_len[b] - 3) / 2 + 1 - 3) / 2 + 1, b < B. */
typedef struct m3_conv1_desc {
  const float* feat; const float* w9c; const float* bias; const float* cmvn_mean; const float* cmvn_istd;
  int32_t B, T, idim, C, act;
  float* out;
  const int32_t* feat_len; int32_t* lens_out;
} m3_conv1_desc;
int m3_subsample_conv1_pair(const m3_conv1_desc* a, const m3_conv1_desc* b, m3_stream stream);
/* The first conv with input channels (conv_subsample_in_ch of the reference, layer/subsampling.py:23-36: (B, T, idim) viewed as
 * (B, in_ch, T, idim / in_ch) -- e.g. static | delta | delta-delta blocks as three image channels of Conv2d(in_ch, C, 3, 2)).
 * m3_conv1_ch_desc is m3_conv1_desc plus in_ch (1..3, idim % in_ch == 0, Fc = idim / in_ch >= 3) and out_bf16 (!= 0: out
 * holds bf16).  idim stays the row width of feat and of cmvn_mean / cmvn_istd; w9c is [in_ch * 9][C] with row ch * 9 + kh * 3 +
 * kw (the (C, in_ch, 3, 3) weight reshaped to (C, in_ch * 9) and transposed); out is [B][T1][F1][C] with F1 = (Fc - 3) / 2 + 1.
 * in_ch = 1 is m3_subsample_conv1_cmvn / m3_conv2d_3x3s2_first bit for bit.  m3_subsample_conv1_ch_pair: the two problems also
 * share in_ch, or the call is refused (run two launches). */
typedef struct m3_conv1_ch_desc {
  const float* feat; const float* w9c; const float* bias; const float* cmvn_mean; const float* cmvn_istd;
  int32_t B, T, idim, C, act;
  float* out;
  const int32_t* feat_len; int32_t* lens_out;
  int32_t in_ch, out_bf16;
} m3_conv1_ch_desc;
int m3_subsample_conv1_ch(const m3_conv1_ch_desc* d, m3_stream stream);
int m3_subsample_conv1_ch_pair(const m3_conv1_ch_desc* a, const m3_conv1_ch_desc* b, m3_stream stream);

/* The packed-row and bf16-row operand forms of the block kernels (what the engine runs on ragged batches, packed_rows, and in
 * the 16-bit modes of long batches), exposed so that they can be tested at the boundary (additions only;
 * tests/test_packed_forms_gpu.py).  Each entry fills the record the engine fills and makes ONE call of the launcher the single
 * entry of its operator makes: no new kernel, no new decision.
 *
 * Packed rows.  A ragged batch of B utterances with len[b] valid frames out of T keeps its live frames back to back: utterance
 * b owns rows [row0[b], row0[b] + min(max(len[b], 0), T)), P = row0[B] rows in all (a device value), and pad_of[p] = b T + t
 * names the padded row of packed row p (-1 for P <= p < B T).
 * m3_pack_plan: len [B] -> row0 [B + 1], pad_of [B * T]; one work-group, 1 <= B <= 1024, T >= 1.  feat_len != NULL: len is an
 * OUTPUT too, len[b] = ((feat_len[b] - 3) / 2 + 1 - 3) / 2 + 1 in C int arithmetic (as m3_subsample_conv1_pair writes lens_out),
 * stored as computed; the clamp to [0, T] applies to the rows alone.
 * m3_unpack_rows: out [B * T][n] dense <- in [P][n] dense: out[b T + t] = in[row0[b] + t] for t < row0[b + 1] - row0[b], zeros
 * beyond.  n >= 1, any value (element copies). */
int m3_pack_plan(int32_t* len, int B, int T, int32_t* row0, int32_t* pad_of, const int32_t* feat_len, m3_stream stream);
int m3_unpack_rows(const float* in, const int32_t* row0, int B, int T, int n, float* out, m3_stream stream);
/* m3_linear_live_rows: m3_linear_ws with a device-side count of live rows, *live_rows_dev = P (0 <= P <= M).  Work-groups whose
 * first row lies beyond P exit: rows 0 .. P (the row AT the count included) hold what m3_linear_ws gives, bit for bit, and
 * every later row either holds that too or is left unwritten -- from the first multiple of the kernel's row tile (16 .. 128
 * rows) above P on, unwritten.  Rows up to M must exist in every operand all the same (their loads may be requested).  The
 * split-K form (a workspace of m3_linear_workspace_size bytes) computes every row.  live_rows_dev: 4-byte aligned, not NULL.
 * m3_linear_live_rows_kernel: host only, as m3_linear_kernel (the count does not change the choice). */
int m3_linear_live_rows(const m3_linear_desc* desc, const int32_t* live_rows_dev, void* workspace, size_t workspace_bytes,
                        m3_stream stream);
const char* m3_linear_live_rows_kernel(const m3_linear_desc* desc, int with_workspace);
/* m3_moe_router_live_rows: m3_moe_router with such a count; its row tile has 16 rows. */
int m3_moe_router_live_rows(const float* embed, int ld_embed, int embed_dim, const float* x, int ldx, int idim, const float* w,
                            const float* bias, const float* ln_gamma, const float* ln_beta, float ln_eps, float* xn, int ld_xn,
                            float* logits, int ld_logits, int S, int num_expert, const int32_t* live_rows_dev, m3_stream stream);
/* m3_conv2d_3x3s2_frames: m3_conv2d_3x3s2 (w_bf16 != 0: w holds bf16, C a multiple of 32) with frames_dev [B], the valid OUTPUT
 * frames per utterance (device int32; NULL: every frame).  The rows (b, t2, f2) with t2 < frames_dev[b] hold what the call
 * without frames_dev gives, bit for bit; a row tile of the LDS-tiled kernels that lies inside one utterance and starts at a frame
 * t2 >= frames_dev[b] is left unwritten (the other kernels of the family compute every row).  in / w / out 16-byte aligned.
 * m3_conv2d_3x3s2_kernel: host only, the name of the kernel the conv runs (with_workspace: as m3_linear_kernel), NULL with the
 * reason in m3_last_error() for a shape the family does not take. */
int m3_conv2d_3x3s2_frames(const float* in, const void* w, const float* bias, int B, int T1, int F1, int C, int act,
                           const int32_t* frames_dev, int w_bf16, float* out, m3_stream stream);
const char* m3_conv2d_3x3s2_kernel(int B, int T1, int F1, int C, int act, int w_bf16, int with_workspace);
/* m3_relpos_attention_packed: m3_relpos_attention_chunk on packed rows.  desc as m3_relpos_attention_pair takes it (len not
 * NULL); with row0 [B + 1] (m3_pack_plan) qkv and out hold the P packed rows, utterance b at rows row0[b] ..., and nothing past
 * an utterance's last frame is read or written; row0 NULL: the padded layout.  out_bf16 != 0: out receives bf16 ([rows][ldo],
 * ldo in elements), the bf16 rounding of the fp32 result.  Strides as m3_relpos_attention.
 * m3_relpos_attention_bf16_packed: m3_relpos_attention_bf16 likewise (desc->qkv and desc->out point at bf16 rows; T <= 128). */
int m3_relpos_attention_packed(const m3_attention_desc* desc, const int32_t* row0, int out_bf16, m3_stream stream);
int m3_relpos_attention_bf16_packed(const m3_attention_desc* desc, const int32_t* row0, m3_stream stream);
/* m3_dwconv_ln_silu_packed: the depthwise conv of m3_dwconv_ln_silu_pair's descriptor (one problem; ldz, gate_sigmoided and
 * left_fill as there) on packed rows.  pad_of / row0 / row_len (= len) as m3_pack_plan leaves them, all three or none (none:
 * the padded layout).  z holds the P packed rows AND, at row P, the pad row: what every frame len[b] <= t < T of the padded
 * layout holds (taps outside [0, T) are the conv's zeros, or left_fill on the left of the causal form), so z has P + 1 rows
 * (B T + 1 when every frame is live); out [P][D] dense, rows at and past P are not written.  out_bf16 != 0: out receives bf16
 * (not with ldz > 0).  Every operand 16-byte aligned. */
int m3_dwconv_ln_silu_packed(const m3_dwconv_desc* desc, const int32_t* pad_of, const int32_t* row0, const int32_t* row_len,
                             int out_bf16, m3_stream stream);
/* m3_layer_norm_ex: m3_layer_norm (dim a multiple of 4, <= 2048; y may alias x) with its optional side results, each NULL or
 * given: y_bf16 [rows][dim] the bf16 rounding of y; y_stats [rows][4][2] (needs y_bf16) the (sum, sum of squares) of the bf16
 * values of a row in part 0 and zeros in parts 1 .. 3 (the ln_stats operand of m3_linear_desc, ln_stat_parts = 4); gamma2 /
 * beta2 / eps2 / y2: a second LayerNorm of the fp32 values y holds, y2 = LN2(y), in the same launch (all of gamma2, beta2, y2
 * or none).  Every operand dense and 16-byte aligned.
 * m3_row_stats_bf16: such statistics of a dense bf16 matrix xb [rows][dim], dim a multiple of 8.
 * m3_rows_to_bf16: xb [S][dim] dense bf16 <- x [S][ldx] fp32, round to nearest even; dim a multiple of 4, ldx >= dim a multiple
 * of 4; x 16-byte, xb 8-byte aligned. */
int m3_layer_norm_ex(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int dim, void* y_bf16,
                     float* y_stats, const float* gamma2, const float* beta2, float eps2, float* y2, m3_stream stream);
int m3_row_stats_bf16(const void* xb, int rows, int dim, float* stats, m3_stream stream);
int m3_rows_to_bf16(const float* x, int ldx, int S, int dim, void* xb, m3_stream stream);

/* Front / back end of the acoustic score.  Global CMVN: y = (x - mean[d]) * istd[d] on frames
 * t < len[b] (the reference's unfinished CmvnPlugin, incomplete_plugin/cmvn_plugin/cmvn_plugin.cu:17-43).
 * Score: y = log_softmax(x) + bias per row, bias = -log(prior) (builder.py:77-88, prior_prob_kernel.cu:11-26). */
int m3_cmvn(const float* x, const int32_t* len, const float* mean, const float* istd, int B, int T, int D, float* y,
            m3_stream stream);
int m3_log_softmax_bias(const float* x, const float* bias, float* y, size_t rows, int n, m3_stream stream);

/* After the encoder: CTC search on the logits.
 * Greedy (model/encoder.py:156-180): ids = argmax over V per frame (first maximum wins), then per utterance drop repeats
 * and blanks over frames t < len[b] (len NULL = all T).  frame_ids [B*T] receives the per-frame argmax (also the
 * kernel's scratch), tokens [B][T] the collapsed ids padded with -1, n_tokens [B] their counts.  All device pointers. */
int m3_ctc_greedy(const float* logits, const int32_t* len, int B, int T, int V, int blank, int32_t* frame_ids,
                  int32_t* tokens, int32_t* n_tokens, m3_stream stream);
/* First beam prune of the prefix beam search on the device (encoder.py:224-231): per row log_softmax, then the k best
 * (value desc, index asc) -> top_logp / top_idx [rows][k]. */
int m3_ctc_topk(const float* logits, size_t rows, int V, int k, float* top_logp, int32_t* top_idx, m3_stream stream);
/* The prefix recursion and second prune (encoder.py:232-275) -- a HOST routine over HOST copies of m3_ctc_topk's output
 * for one utterance of T frames.  Writes at most `beam` hypotheses, best first: hyp_tokens [beam][T] (-1 padded),
 * hyp_len [beam], hyp_score [beam] = log(p_blank + p_non_blank), *n_hyps. */
int m3_ctc_prefix_beam_search(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                              int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, int32_t* n_hyps);
/* The same search on the DEVICE, for B utterances at once and resumable at any frame boundary (csrc/ctc_beam.hip).  The
 * result equals m3_ctc_prefix_beam_search on each utterance's frames: same prefixes in the same order, scores from the same
 * double-precision recursion.  One work-group per utterance; the search state (beam, prefix trie, canonical-node hash
 * table) lives in caller-owned device memory of m3_ctc_beam_state_size bytes.  Limits: 1 <= beam <= 32, 1 <= k <= 32
 * (the reference uses k = beam); max_frames bounds the frames one search may consume over its lifetime.
 * m3_ctc_beam_state_size: host-only; 0 (and m3_last_error) on a bad descriptor.
 * m3_ctc_beam_reset: every utterance back to the empty prefix (pb = 0, pnb = -inf), no frame consumed.
 * m3_ctc_beam_advance: top_logp / top_idx [B][T_chunk][k] (m3_ctc_topk's output), n_frames [B] (device) = how many of
 *   utterance b's T_chunk rows are real (clamped to [0, T_chunk]; the rest is padding).  All frames run in one launch, no
 *   host sync.  An advance that would take an utterance past max_frames consumes nothing and marks it failed (nothing is
 *   written outside the state); the failure is sticky until the next reset.
 * m3_ctc_beam_nbest: hyp_tokens [B][beam][max_frames] (-1 padded), hyp_len [B][beam], hyp_score [B][beam] =
 *   log(p_blank + p_non_blank) (-inf for unused rows), n_hyps [B] (-1 for a failed utterance); best first.  All device. */
typedef struct m3_ctc_beam_desc {
  int32_t B;
  int32_t beam;
  int32_t k;
  int32_t max_frames;
  int32_t blank;
} m3_ctc_beam_desc;
size_t m3_ctc_beam_state_size(const m3_ctc_beam_desc* desc);
int m3_ctc_beam_reset(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, m3_stream stream);
/* The same for the n utterances listed in `slots` (device int32[n]; entries outside [0, B) are skipped), one launch: the
 * other searches of the state go on untouched. */
int m3_ctc_beam_reset_slots(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                            m3_stream stream);
int m3_ctc_beam_advance(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const float* top_logp,
                        const int32_t* top_idx, int T_chunk, const int32_t* n_frames, m3_stream stream);
int m3_ctc_beam_nbest(const m3_ctc_beam_desc* desc, const void* state, size_t state_bytes, int32_t* hyp_tokens,
                      int32_t* hyp_len, float* hyp_score, int32_t* n_hyps, m3_stream stream);
/* Context biasing of the prefix beam search (hotwords; csrc/ctc_beam.hip, csrc/decode.hip).  The searches know a weighted
 * deterministic token automaton, nothing about phrases: cls [V] int32 maps a token to a column in [0, A) (0 = in no phrase),
 * next [n_states][A] int32 is total (state 0 is the start), delta [n_states][A] float32 is added to the prefix's bonus on
 * that arc, pot [n_states] float32 is the part of the bonus that is still provisional in that state.  For a prefix y,
 * state(y) and bonus(y) come from walking y from state 0, the bonus summed in double left to right; final(y) = bonus(y) -
 * pot[state(y)].  The second prune ranks by log(p_blank + p_non_blank) + bonus (first-touch tie-break as before); the
 * hypotheses are reported ordered by log(p_blank + p_non_blank) + final, stable on the beam order.
 * A CONTEXT SET is one image of 4-byte little-endian words holding G >= 0 graphs:
 *   [0x5843334d, G, V, words]   G x [n_states, A, cls, next, delta, pot, 0, 0]   the tables
 * (cls .. pot: word offsets of the graph's tables from the start of the image).  Limits: G <= 1024, n_states <= 65536,
 * A <= min(V + 1, 65536), image <= 64 MiB.  m3asr.context (Python) compiles phrase lists into such images.
 * m3_ctc_context_validate: host-only check of a HOST image for vocabulary size V: header, limits, every table inside the
 *   image, every cls entry in [0, A), every next entry in [0, n_states), delta and pot finite.  Run it on the host copy
 *   before the image is uploaded; the device search only sees images that passed.  Independently the kernels range-check
 *   graph_of, the header and every index they form an address from (a failed check means "unbiased" / column 0 / state 0).
 * m3_ctc_prefix_beam_search_ctx: m3_ctc_prefix_beam_search with the biased ranking, one utterance, graph `graph` of a host
 *   image (validated inside the call).  Adds hyp_bonus [beam] (= final) and hyp_state [beam]; hyp_score stays the CTC score.
 *   image NULL (or graph -1): exactly what m3_ctc_prefix_beam_search returns, bonus and state 0.
 * m3_ctc_beam_ctx_*: the device search with the biased ranking.  The state is m3_ctc_beam_state_size bytes laid out as for
 *   m3_ctc_beam_*, byte for byte, then per utterance ctx_state [1 + max_frames * beam] int32 and ctx_bonus [...] double
 *   (every trie node's context state and bonus: a prefix that leaves the beam and returns finds them again).
 *   _advance / _nbest take the DEVICE image (NULL, 0 = no graphs) and graph_of [B] (device int32; a value outside [0, G),
 *   -1 by convention, = this utterance is unbiased, and its result is m3_ctc_beam_*'s bit for bit).  An utterance keeps one
 *   graph from a reset to the next.  _nbest additionally writes hyp_bonus [B][beam] (= final). */
int m3_ctc_context_validate(const void* image, size_t image_bytes, int V);
int m3_ctc_prefix_beam_search_ctx(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                  const void* image, size_t image_bytes, int graph, int32_t* hyp_tokens, int32_t* hyp_len,
                                  float* hyp_score, float* hyp_bonus, int32_t* hyp_state, int32_t* n_hyps);
size_t m3_ctc_beam_ctx_state_size(const m3_ctc_beam_desc* desc);
int m3_ctc_beam_ctx_reset(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, m3_stream stream);
int m3_ctc_beam_ctx_reset_slots(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                                m3_stream stream);
int m3_ctc_beam_ctx_advance(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const void* image, size_t image_bytes,
                            const int32_t* graph_of, const float* top_logp, const int32_t* top_idx, int T_chunk,
                            const int32_t* n_frames, m3_stream stream);
int m3_ctc_beam_ctx_nbest(const m3_ctc_beam_desc* desc, const void* state, size_t state_bytes, const void* image,
                          size_t image_bytes, const int32_t* graph_of, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score,
                          float* hyp_bonus, int32_t* n_hyps, m3_stream stream);
/* N-gram LM shallow fusion of the prefix beam search: a prefix y is ranked by
 *   (ctc + bonus) + (alpha lm(y) + beta |y|),   lm(y) = log P_LM(y), natural log.
 * An LM IMAGE is one image of 4-byte little-endian words: a 20-word header
 *   [0x4d4c334d, version = 1, V, order, n_states, n_arcs, start, unk_logp (float bits),
 *    word offsets of uni_logp, uni_next, arc_begin, arc_tok, arc_next, arc_logp, bo_state, bo_weight, final, words, 0, 0]
 * and the tables of a deterministic back-off automaton over context states: state 0 (the empty context) has dense arcs
 * uni_logp [V] float / uni_next [V] int32; state s >= 1 has the sparse arcs [arc_begin[s], arc_begin[s + 1]) of arc_tok
 * (strictly ascending inside a state), arc_next, arc_logp, and backs off to bo_state[s] < s at the price bo_weight[s];
 * final [n_states] = log P(</s> | state), back-off resolved.  Limits: order <= 8, n_states <= 2^26, image <= 1 GiB.
 * m3asr.lm (Python) compiles ARPA files into such images.  THE SCORE CONTRACT, step(state, tok):
 *   w = 0.0 (double); st = state; while st != 0: binary-search tok among st's arcs; found: return (w + (double)arc_logp,
 *   arc_next); else w += (double)bo_weight[st], st = bo_state[st].  At st = 0: (w + (double)uni_logp[tok], uni_next[tok]);
 *   a token outside [0, V): (w + (double)unk_logp, 0).
 * lm(y) is the left-to-right double sum of the steps from `start`; lm_state(y) the state reached.
 * m3_ctc_lm_validate: host-only check of a HOST image for vocabulary size V: header, limits, every table inside the image,
 *   arc_begin monotone from 0 to n_arcs, arc_tok ascending inside a state and in [0, V), every uni_next / arc_next in
 *   [0, n_states), bo_state[s] < s and at most order - 1 back-off levels above state 0, every float finite.  Run it on the
 *   host copy before the image is uploaded.  Independently the kernels range-check the header and every index they form an
 *   address from (a failed header check means "LM off", a bad index state 0).
 * m3_ctc_prefix_beam_search_lm: m3_ctc_prefix_beam_search_ctx plus a host LM image (validated inside the call), alpha, beta
 *   and use_eos.  Candidates are pruned by the key above, evaluated in double in exactly that association; the hypotheses come
 *   out ordered by (ctc + final) + (alpha (lm + final_lm[lm_state] use_eos) + beta |y|), stable on the beam order.  hyp_score
 *   stays the CTC score, hyp_bonus the context final; hyp_lm [beam] = lm + final_lm use_eos.  lm_image NULL: exactly what
 *   m3_ctc_prefix_beam_search_ctx returns (hyp_lm, if given, zeros).
 * m3_ctc_beam_lm_*: the device search with the fused ranking.  The state is m3_ctc_beam_ctx_state_size bytes laid out as for
 *   m3_ctc_beam_ctx_*, byte for byte, then per utterance lm_state [1 + max_frames * beam] int32 and lm_sum [...] double.
 *   _advance / _nbest take both DEVICE images (either may be NULL, 0), graph_of [B] as m3_ctc_beam_ctx_*, lm_on [B] (device
 *   int32; 0 = this utterance runs without the LM, and its result is m3_ctc_beam_ctx_*'s bit for bit) and alpha, beta (and
 *   _nbest use_eos): run-time arguments, not part of the image.  An utterance keeps its lm_on, alpha and beta from a reset to
 *   the next.  _nbest additionally writes hyp_lm [B][beam].
 * AN LM SET is one image of 4-byte little-endian words holding G complete LM images, so that every utterance of
 * a batch or a pool of streams picks its own LM:
 *   [0x534c334d, version = 1, V, G, total words, 0, 0, 0]   G x [offset words, n words, scale (float bits), 0]   the members
 * Each member is an LM image as above, byte for byte, over the set's V; it starts at `offset words` from the start of the set,
 * a multiple of 4 (members stay 16-byte aligned); members come in ascending order and do not overlap.  Limits: 1 <= G <= 64,
 * every member within the single image's limits, the set <= 2 GiB; scale finite and > 0.
 * Every DEVICE entry point that takes an lm_image (m3_ctc_beam_lm_advance / _nbest, m3_aed_ngram_score, m3_aed_bias_score)
 * takes either kind, told apart by word 0.  With a single image lm_on[b] != 0 means "on", as above.  With a set lm_on[b] = j,
 * 1 <= j <= G, picks member j - 1; 0 and every other value mean "off" (the rule of graph_of).  The utterance's LM weight is
 * alpha * (double)scale_j, one double product (scale 1.0 changes no bit); beta and use_eos are the call's.  The kernels resolve
 * (member, words, scale) once per utterance and range-check the set's header and the directory entry like a single header: a
 * bad set header means "LM off" for every utterance, a bad entry or member header for that utterance, a bad index inside a
 * member state 0.  The device calls admit lm_bytes up to the set's 2 GiB, since only the device copy says which kind it is; a
 * SINGLE image above its own 1 GiB limit runs as "LM off" (the kernels check it where they read word 0).  The start state is the member's: a search restarted with another member begins from that member's start.
 * m3_ctc_lm_validate takes either kind of HOST image; of a set it checks the header, the directory (alignment, order, bounds,
 *   scale) and every member by the rules above.
 * m3_ctc_ngram_set_member: host only; member j in [0, G) of a host set (validated inside the call): *member points into `image`,
 *   *member_bytes is its size, *scale (may be NULL) its scale -- what m3_ctc_prefix_beam_search_lm takes as its lm_image. */
int m3_ctc_lm_validate(const void* image, size_t image_bytes, int V);
int m3_ctc_ngram_set_member(const void* image, size_t image_bytes, int j, const void** member, size_t* member_bytes, float* scale);
int m3_ctc_prefix_beam_search_lm(const float* top_logp, const int32_t* top_idx, int T, int k, int beam, int blank,
                                 const void* image, size_t image_bytes, int graph, const void* lm_image, size_t lm_bytes,
                                 double alpha, double beta, int use_eos, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score,
                                 float* hyp_bonus, int32_t* hyp_state, float* hyp_lm, int32_t* n_hyps);
size_t m3_ctc_beam_lm_state_size(const m3_ctc_beam_desc* desc);
int m3_ctc_beam_lm_reset(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, m3_stream stream);
int m3_ctc_beam_lm_reset_slots(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                               m3_stream stream);
int m3_ctc_beam_lm_advance(const m3_ctc_beam_desc* desc, void* state, size_t state_bytes, const void* image, size_t image_bytes,
                           const int32_t* graph_of, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha,
                           double beta, const float* top_logp, const int32_t* top_idx, int T_chunk, const int32_t* n_frames,
                           m3_stream stream);
int m3_ctc_beam_lm_nbest(const m3_ctc_beam_desc* desc, const void* state, size_t state_bytes, const void* image, size_t image_bytes,
                         const int32_t* graph_of, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha,
                         double beta, int use_eos, int32_t* hyp_tokens, int32_t* hyp_len, float* hyp_score, float* hyp_bonus,
                         float* hyp_lm, int32_t* n_hyps, m3_stream stream);
/* Greedy search chunk by chunk: per stream the previous frame's argmax is carried across calls and the collapsed tokens are
 * appended to a buffer inside the state (m3_ctc_greedy_stream_state_size bytes, device).  After any sequence of advances the
 * tokens equal m3_ctc_greedy on the concatenation of the frames each stream was given.
 * m3_ctc_greedy_stream_advance: logits [B][T_chunk][V], n_frames [B] (device) real rows per stream, frame_ids [B*T_chunk]
 *   device scratch (receives the per-frame argmax).  Past max_frames the stream consumes nothing and is marked failed.
 * m3_ctc_greedy_stream_tokens: tokens [B][max_frames] (-1 padded), n_tokens [B] (-1 for a failed stream).  All device. */
typedef struct m3_ctc_greedy_desc {
  int32_t B;
  int32_t max_frames;
  int32_t blank;
} m3_ctc_greedy_desc;
size_t m3_ctc_greedy_stream_state_size(const m3_ctc_greedy_desc* desc);
int m3_ctc_greedy_stream_reset(const m3_ctc_greedy_desc* desc, void* state, size_t state_bytes, m3_stream stream);
int m3_ctc_greedy_stream_reset_slots(const m3_ctc_greedy_desc* desc, void* state, size_t state_bytes, const int32_t* slots,
                                     int n, m3_stream stream); /* only the n streams listed in `slots` (device int32[n]) */
int m3_ctc_greedy_stream_advance(const m3_ctc_greedy_desc* desc, void* state, size_t state_bytes, const float* logits,
                                 int T_chunk, int V, const int32_t* n_frames, int32_t* frame_ids, m3_stream stream);
int m3_ctc_greedy_stream_tokens(const m3_ctc_greedy_desc* desc, const void* state, size_t state_bytes, int32_t* tokens,
                                int32_t* n_tokens, m3_stream stream);
/* Endpoint detection next to the two searches (csrc/ctc_beam.hip): when is an utterance over.  Frames are
 * encoder output frames.  Per stream the state is (frames, trailing_blank, decoded, first_speech, last_speech, fired_rule,
 * fired_frame), after a reset (0, 0, 0, -1, -1, 0, -1).  Each real frame, in order, is judged by entry 0 of m3_ctc_topk's
 * output for it (the argmax, the greedy search's winner):  frames += 1;  the frame is BLANK iff top_idx0 == blank and
 * top_logp0 > log_blank_threshold (strict): trailing_blank += 1, any other frame sets trailing_blank = 0;  top_idx0 != blank
 * sets decoded = 1, last_speech = frames - 1 and first_speech if it was -1.  Then rule r = 1 .. n_rules fires iff
 * (decoded || !must_decoded) && trailing_blank >= min_trailing && frames >= min_length; the first that fires latches
 * fired_rule = r, fired_frame = frames - 1, and from then on no frame changes anything until the stream is reset.
 * Limits: 1 <= n_rules <= 4, counts >= 0, must_decoded 0 or 1, log_blank_threshold in [log 0.5, 0) as a float32 (a blank above
 * p = 0.5 is necessarily entry 0, for any k >= 1).  The state is eight words per stream (m3_ctc_endpoint_state_size bytes,
 * device) and there is no max_frames: this is the one piece of a session that never overflows.
 * m3_ctc_endpoint_advance: top_logp / top_idx [B][T_chunk][k], n_frames [B] (device) real rows per stream, clamped to
 *   [0, T_chunk]; rows past it are padding and are not read, a stream with 0 frames keeps its state word for word.  One wave
 *   per stream, no host sync.
 * m3_ctc_endpoint_read: info [B][8] (device int32) = the seven values above in that order and one spare word (0). */
typedef struct m3_ctc_endpoint_rule {
  int32_t must_decoded;
  int32_t min_trailing;
  int32_t min_length;
} m3_ctc_endpoint_rule;
typedef struct m3_ctc_endpoint_desc {
  int32_t B;
  int32_t blank;
  int32_t n_rules;
  float log_blank_threshold;
  m3_ctc_endpoint_rule rule[4];
} m3_ctc_endpoint_desc;
size_t m3_ctc_endpoint_state_size(const m3_ctc_endpoint_desc* desc);
int m3_ctc_endpoint_reset(const m3_ctc_endpoint_desc* desc, void* state, size_t state_bytes, m3_stream stream);
int m3_ctc_endpoint_reset_slots(const m3_ctc_endpoint_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                                m3_stream stream); /* only the n streams listed in `slots` (device int32[n]) */
int m3_ctc_endpoint_advance(const m3_ctc_endpoint_desc* desc, void* state, size_t state_bytes, const float* top_logp,
                            const int32_t* top_idx, int T_chunk, int k, const int32_t* n_frames, m3_stream stream);
int m3_ctc_endpoint_read(const m3_ctc_endpoint_desc* desc, const void* state, size_t state_bytes, int32_t* info,
                         m3_stream stream);
/* CTC forced alignment (csrc/ctc_align.hip): WHEN each token of a given hypothesis was spoken.  For every one of n
 * utterances, given its frames' logits and ANY token sequence (however it was found: CTC search, rescoring, attention
 * decoding), the best CTC alignment -- Viterbi over the blank-interleaved trellis -- and from it each token's first frame, end
 * frame, peak frame and peak log-posterior.  Additions only (the ABI version stays 10); replaces nothing in the reference,
 * which has no aligner.
 * Utterances are packed and ragged: utterance u has T = n_frames[u] frames, its logits are the rows row0[u] .. row0[u] + T of
 * `logits` (a padded (B, T, V) batch is row0[u] = u * T), its tokens y[0 .. L) = tokens[tok0[u] .. tok0[u + 1]) (tok0 [n + 1] =
 * prefix sums of the token counts).  row0, n_frames, tokens, tok0 are device int32.
 * THE CONTRACT (restated in tests/ctc_align_ref.py), e[t][v] = log_softmax(logits row t)[v], S = 2 L + 1 states, lab(s) = blank
 * for even s and y[s >> 1] for odd s:
 *   a[0][0] = e[0][blank], a[0][1] = e[0][y[0]], every other state -inf;  a[t][s] = best + e[t][lab(s)], best over
 *   stay a[t-1][s] | step a[t-1][s-1] (s >= 1) | skip a[t-1][s-2] (s odd, s >= 3, lab(s) != lab(s-2)); a later move replaces an
 *   earlier one only when STRICTLY greater (ties: stay over step over skip, -inf against -inf included); one float32 add on a
 *   float32 maximum per (t, s).  The path ends in state S - 1, or in S - 2 when S > 1 and a[T-1][S-2] > a[T-1][S-1] (strictly),
 *   and state[t] follows the recorded moves back.  Token i: start = first frame with state 2 i + 1, end = last such frame + 1,
 *   peak = the frame of [start, end) with the largest e[t][y[i]] (the earliest on ties), peak_logp = that value.
 *   score = a[T-1][final state].  T = 0 with L = 0 is an alignment of score 0.
 * status [n]: 0 ok;  1 no alignment exists (T < L + the number of i with y[i] == y[i-1], T = 0 < L, or a best score of -inf);
 *   2 bad input (a token that is `blank` or outside [0, V), n_frames[u] outside [0, max_frames], more than max_tokens tokens).
 *   For status 1 and 2 the utterance's score is -inf, its state row and its tok_start / tok_end / tok_peak are -1 and its tok_logp
 *   is -inf; nothing outside the utterance's own outputs is written.  Every loop is bounded by T and S, never by a value read
 *   from the logits: a NaN gives an unspecified path, no access out of bounds and no hang.
 * m3_ctc_align_workspace_size: host-only; bytes of the move table (one byte per frame and state).  0 (and m3_last_error) for a
 *   descriptor the library refuses: a negative field, blank outside [0, V), n or max_frames above 2^20, max_tokens above 4000
 *   (two score vectors of S floats live in 64 KB of LDS), sizes that overflow the int32 index arithmetic.  Never 0 otherwise.
 * m3_ctc_align_emit: the only stage that rounds.  One wave per (utterance, frame): fp32 logsumexp over V (maximum subtracted),
 *   then emit[u][t][0] = x[blank] - lse and emit[u][t][1 + i] = x[y[i]] - lse; emit is [n][max_frames][max_tokens + 1] fp32,
 *   dense, and only rows t < T and columns <= L are written (nothing for an utterance whose sizes are bad; -inf for a token
 *   outside [0, V)).  ldl >= V, any value, logits 4-byte aligned (16-byte loads are used where a row's address allows);
 *   logits may hold -inf, a row must hold one finite value.
 * m3_ctc_align_path: exact arithmetic on `emit`.  One work-group per utterance, serial in t, parallel in s.  workspace: at
 *   least m3_ctc_align_workspace_size bytes.  score [n] f32, status [n], state [n][max_frames] (entries at and past T are -1),
 *   tok_start / tok_end / tok_peak (int32) and tok_logp (f32) [tok0[n]], indexed like `tokens`.
 * Both calls are enqueued on `stream` and neither synchronises; emit then path on one stream is the whole operation. */
typedef struct m3_ctc_align_desc {
  int32_t n;
  int32_t V;
  int32_t blank;
  int32_t max_frames;
  int32_t max_tokens;
} m3_ctc_align_desc;
size_t m3_ctc_align_workspace_size(const m3_ctc_align_desc* desc);
int m3_ctc_align_emit(const m3_ctc_align_desc* desc, const float* logits, int ldl, const int32_t* row0, const int32_t* n_frames,
                      const int32_t* tokens, const int32_t* tok0, float* emit, m3_stream stream);
int m3_ctc_align_path(const m3_ctc_align_desc* desc, const float* emit, const int32_t* n_frames, const int32_t* tokens,
                      const int32_t* tok0, void* workspace, size_t ws_bytes, float* score, int32_t* status, int32_t* state,
                      int32_t* tok_start, int32_t* tok_end, int32_t* tok_peak, float* tok_logp, m3_stream stream);

/* Streaming operators of the reference's plugin library (built there but not registered, trt_plugin_plus.cpp:155-156).
 * CatSplitCachePluginDynamic (cat_split_cache_kernel.cu:30-107), 4-byte elements: output [B][cache_dim+input_dim] =
 * in_cache ++ input, out_cache [B][cache_dim] = the last cache_dim values of output. */
int m3_cat_split_cache(const void* in_cache, const void* input, int B, int cache_dim, int input_dim, void* output,
                       void* out_cache, m3_stream stream);
/* AttStreamSoftmaxPluginDynamic (att_stream_softmax_kernel.cu:28-191): scores [B][N][ld]; row (b,n) valid on
 * [max(0, ld - decode_frame_num[b]), min(ld, min(ld, mask_idx[b]) + cache_len)); out = exp((x - max) * scale) / sum
 * there, 0 elsewhere. */
int m3_att_stream_softmax(const float* scores, const int32_t* decode_frame_num, const int32_t* mask_idx, int B, int N,
                          int ld, int cache_len, float scale, float* out, m3_stream stream);
/* RelPositionalEncodingPluginDynamic (rel_positional_encoding_kernel.cu:62-69; streaming contract :108-111):
 * y = x * scale on (B,T,D); pos_emb [T][D] = pe[off : off+T], off = frame_num[0] (device int32 [B]; NULL = 0);
 * frame_num_out[b] = frame_num[b] + T (distinct buffer; may be NULL).  pe has pe_len positions; max_offset is the
 * caller's bound on frame_num[0], checked against pe_len on the host. */
int m3_rel_positional_encoding(const float* x, const float* pe, int pe_len, const int32_t* frame_num, int max_offset,
                               float scale, int B, int T, int D, float* y, float* pos_emb, int32_t* frame_num_out,
                               m3_stream stream);

/* small plugins */
int m3_att_masked_softmax(const float* scores, const int32_t* len, int B, int H, int T1, int T2, float scale,
                          float* out, m3_stream stream);                 /* att_masked_softmax_plugin.cpp:84-108 */
int m3_masked_fill(const float* x, const int32_t* len, int B, int C, int T, float fill, float* y,
                   m3_stream stream);                                     /* masked_fill_plugin.cpp:87-108 */
int m3_glu(const float* x, int outer, int C, int inner, float* y, m3_stream stream); /* glu_plugin.cpp:90-134 */
int m3_mask_conv2d_sample(const int32_t* len_in, int B, int left_padding, int stride, int32_t* len_out,
                          m3_stream stream);                              /* mask_conv2d_sample_plugin.cpp:70-80 */
int m3_scale(const float* x, float scale, float* y, size_t n, m3_stream stream); /* rel_positional_encoding_kernel.cu:62-69 */

/* TensorRT-native element-wise / shuffle / concat / matmul layers used through network_helper */
int m3_unary(const float* x, float* y, size_t n, int act, m3_stream stream);
int m3_binary(const float* a, const float* b, float* y, const int64_t* shape, const int64_t* strides_a,
              const int64_t* strides_b, int ndim, int op, m3_stream stream);
int m3_permute(const float* x, float* y, const int64_t* out_shape, const int64_t* in_strides, int ndim,
               m3_stream stream);
int m3_concat_last(const float* a, int da, const float* b, int db, float* y, size_t rows, m3_stream stream);
int m3_softmax(const float* x, float* y, size_t rows, int n, m3_stream stream);
int m3_batched_matmul(const float* a, const float* b, float* c, int batch, int M, int N, int K,
                      int64_t stride_a, int64_t stride_b, int transpose_b, m3_stream stream);
/* zero padding of the last two dims (TensorRT IPaddingLayer; network.add_padding of the causal conv module,
 * convolution.py:118-123): x (outer, H, W) -> y (outer, H + pre_h + post_h, W + pre_w + post_w) */
int m3_pad2d(const float* x, size_t outer, int H, int W, int pre_h, int post_h, int pre_w, int post_w, float* y,
             m3_stream stream);
/* (B,C,T) -> (B,C,T + 2 pad - K + 1), as nn.Conv1d(groups = C, padding = pad) */
int m3_depthwise_conv1d(const float* x, const float* w, const float* bias, int B, int C, int T, int K, int pad,
                        float* y, m3_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-encoder engine.  Replaces the TensorRT engine built by builder.py:36-98 and run by
 * infer.py:38-103 (IExecutionContext::execute_v2): feat (B,T,idim) f32 + feat_len (1,B) i32 -> logits (B,T',V).
 * The weight blob is the "plan" payload produced by the builder (packed fp32, offsets in `table`).
 * ---------------------------------------------------------------------------------------------- */
typedef struct m3_engine m3_engine;

typedef struct m3_engine_config {
  int32_t input_dim, output_dim;
  int32_t attention_dim, attention_heads, num_blocks;
  int32_t embed_dim, embed_heads, embed_linear_units, embed_blocks;
  int32_t num_experts, hidden_units;
  int32_t cnn_module_kernel;
  int32_t cnn_layer_norm;        /* 1 = LayerNorm in the conv module, 0 = (folded) batch norm */
  int32_t embed_cnn_layer_norm;
  int32_t router_with_bias, keep_expert_output;
  int32_t ep_world_size, ep_rank; /* expert parallel: this rank owns experts [rank*E_loc, (rank+1)*E_loc) */
  int32_t fold_pos_proj;         /* 1 = linear_pos(pos_emb) computed once per T' at shape set-up */
  int32_t debug_taps;            /* 1 = keep every block's output (the reference's DumpTensor taps) */
  int32_t log_softmax_out;       /* 1 = output log_softmax(logits) (+ "output_bias" weight entry if present, e.g. -log prior) */
  int32_t fuse_route;            /* 1 = router + SoftmaxTopK + ScatterMapping in one launch per layer (S <= 256, 1 rank);
                                  * 2 = split route: embed half of all routers in one GEMM, x half with folded LayerNorm,
                                  *     norm_ff applied by the expert kernel (1 rank, fp32) */
  int32_t shape_cache;           /* bound (shape, buffers) sets kept besides the current one, each with its stage list and
                                  * captured hipGraph (LRU): 0 = default 7, -1 = none.  Nothing the engine needs between two
                                  * forwards lives in the caller's workspace (the folded positional projection is
                                  * engine-owned device memory), so one workspace may serve every shape. */
  int32_t bf16_activations;      /* 16-bit modes, long batches: activations that only feed GEMMs are kept as bf16 and a bf16
                                  * copy of the residual stream is maintained (0 = automatic, -1 = never; the expert-parallel
                                  * host driver needs -1 because it replaces the stage that writes the copy) */
  int32_t weight_dtype;          /* M3_F32 / M3_BF16: storage of the GEMM weights (linear / point-wise conv /
                                  * conv2 / expert w_1, w_2 / pos_all); router, norms, biases, conv1, depthwise stay fp32.
                                  * M3_FP8: expert w_1 / w_2 in e4m3 with per-row scales ("...w_1.scale", "...w_2.scale"),
                                  * the other GEMM weights bf16.  M3_MXFP4: expert w_1 / w_2 as MXFP4 code bytes with block
                                  * scale bytes ("...w_1.scale", "...w_2.scale"; every such entry has dtype M3_MXFP4), the
                                  * other GEMM weights bf16; attention_dim % 128 == 0, one rank only */
  int32_t packed_rows;           /* ragged batches (B > 1): run every row-wise kernel of the blocks on the sum of the valid
                                  * frames instead of B x T' padded rows (0 = automatic: on for B > 1 on one rank without
                                  * debug taps / fused routing, -1 = never, 1 = also for B = 1).  The interface does not
                                  * change: logits come back as (B, T', V), zeros past each utterance's last frame; the
                                  * "x" / "xn" / "embed" buffers then hold packed rows ("row0" = first row per utterance) */
  int32_t fp8_activations;       /* weight_dtype M3_FP8 only: 1 = fp8 ARITHMETIC in the grouped expert FFN where the fused
                                  * fp8 kernel applies (long batches): rows quantised per row, H with the static per-layer
                                  * scale "blocks.N.feed_forward.experts.h_scale" of the plan (calibrated); elsewhere the
                                  * weight-only form runs */
  int32_t ep_stages;             /* 1 = build the expert-parallel stage list ("blocks.N.moe_ep.send / .expert / .combine")
                                  * even with ep_world_size <= 1: a one-rank rehearsal of the exchange, the two all-to-alls
                                  * being device copies ("moe_ep.exchange1 / 2" stages).  ep_world_size > 1 always builds it */
  int32_t fork_embed;            /* the embed encoder is independent of the main encoder until blocks.0's router reads the
                                  * embedding (conformer_fmoe_..._hier.py:206-215): in the captured hipGraph it runs as a second
                                  * branch beside the main subsampler and block 0's macaron FFN / attention / conv module, on
                                  * its own scratch buffers.  1 = on, 0 / -1 = off (default: with several execution contexts the
                                  * extra branch costs more queue concurrency than it saves latency).  Stage-wise
                                  * runs (m3_engine_run) stay one chain; results are identical either way */
  int32_t static_chunk_size;     /* > 0: static chunk mask in every attention (add_optional_chunk_mask, utils/mask.py:127-134;
                                  * subsequent_chunk_mask :42-75): query frame i sees keys [max((i / c - left) c, 0),
                                  * min((i / c + 1) c, T')) and < len.  0 = full context */
  int32_t num_left_chunks;       /* chunks to the left a query sees with static_chunk_size > 0; < 0: all */
  int32_t causal;                /* 1 = causal ConvolutionModule in the main encoder (convolution.py:43-49,118-123: lorder = K - 1
                                  * frames padded on the left in front of pointwise_conv1, depthwise conv without padding); needs
                                  * the plan entry "blocks.N.conv_module.left_fill" [D] = GLU(pointwise_conv1.bias) */
  int32_t embed_causal;          /* the same for the embed encoder (conformer_embed_domain_acc.py:51,127; embed_conf['causal']) */
} m3_engine_config;

typedef struct m3_weight_entry {
  const char* name; /* packed tensor name, see m3asr/plan.py */
  const void* data; /* device pointer */
  int64_t numel;
  int32_t dtype;    /* enum m3_dtype; checked against what the engine expects for that tensor */
} m3_weight_entry;

m3_engine* m3_engine_create(const m3_engine_config* config, const m3_weight_entry* table, int n_entries);
void m3_engine_destroy(m3_engine* engine);
/* T' for T input frames (MaskConv2dSample twice, mask_conv2d_sample_kernel.cu:34-35) */
int m3_engine_output_frames(int T);
size_t m3_engine_workspace_size(const m3_engine* engine, int B, int T);
/* Enqueue one encoder forward.  All pointers device, caller-owned.  use_graph=1 replays a hipGraph
 * captured for this (B, T, pointers) on first use. */
int m3_engine_forward(m3_engine* engine, const float* feat, const int32_t* feat_len, int B, int T, float* logits,
                      void* workspace, size_t workspace_bytes, int use_graph, m3_stream stream);
/* Staged execution (used by the expert-parallel host driver, m3asr/ep.py, and by per-stage timing):
 * m3_engine_prepare binds shape + caller-owned buffers and builds the ordered kernel-stage list;
 * stages [first, last) are then enqueued with m3_engine_run.  Stage names are
 * "<prefix>.<op>", e.g. "embed.blocks.0.ffn_macaron.w1", "blocks.3.moe_router", "blocks.3.moe_local.expert",
 * "logits"; one kernel per stage.  In expert-parallel mode the host replaces the "blocks.N.moe_local.*" stages by
 * local index -> RCCL all-to-all -> m3_moe_expert_ffn on the received rows -> all-to-all back -> combine. */
int m3_engine_prepare(m3_engine* engine, const float* feat, const int32_t* feat_len, int B, int T, float* logits,
                      void* workspace, size_t workspace_bytes);

/* ---- chunk-by-chunk (streaming) execution -------------------------------------------------------------------------------
 * Decoding-chunk semantics of trainer_3m_fix/model/encoder.py:100-140 (decoding_chunk_size, num_decoding_left_chunks) with
 * the caches the reference's streaming plugins carry (cat_split_cache_kernel.cu:30-107, att_stream_softmax_kernel.cu:136-191,
 * rel_positional_encoding_kernel.cu:108-123).  The engine must have static_chunk_size = c > 0 and causal = embed_causal = 1.
 * B utterances are decoded side by side, one chunk of c output frames per call: the caller hands over the window of
 * m3_engine_chunk_input_frames() = 4c + 3 feature frames that starts at input frame 4 c n (windows overlap by 3 frames, the
 * context of the two stride-2 convs) and, per utterance, how many of its frames are real (0 for an utterance that has ended
 * or has fewer than 7 frames left).  logits (B, c, V): rows past an utterance's valid frames are undefined.
 * State (caller-owned device memory, m3_engine_stream_state_size bytes): a device-side chunk counter, per block the K | V
 * history [B][history_frames][2D] (a ring when num_left_chunks >= 0: history_frames >= (num_left_chunks + 1) c; otherwise it
 * must hold the whole stream) and the depthwise conv's K-1 frame cache.  max_frames bounds the stream's length in output
 * frames (positions; < rows of "pe").  m3_engine_stream_reset starts a new set of B streams.  chunk_index is the host's
 * count of chunks already decoded (validated against max_frames; the kernels use the device-side counter, so the call is a
 * hipGraph replay from the second chunk on).  Contract: chunk n's logits equal rows [n c, (n+1) c) of m3_engine_forward on
 * the whole utterances up to fp32 rounding of the GEMMs. */
typedef struct m3_stream_desc {
  int32_t B;
  int32_t history_frames;
  int32_t max_frames;
} m3_stream_desc;
int m3_engine_chunk_input_frames(const m3_engine* engine);
size_t m3_engine_stream_state_size(const m3_engine* engine, const m3_stream_desc* desc);
int m3_engine_stream_reset(m3_engine* engine, const m3_stream_desc* desc, void* state, size_t state_bytes, m3_stream stream);
int m3_engine_forward_chunk(m3_engine* engine, const m3_stream_desc* desc, void* state, size_t state_bytes,
                            const float* feat_chunk, const int32_t* chunk_feat_len, float* logits, void* workspace,
                            size_t workspace_bytes, int chunk_index, int use_graph, m3_stream stream);
/* ---- slot mode: the B streams of one state start, pause and end independently ---------------------------------------------
 * The calls above move all B streams in lockstep (one chunk counter).  In slot mode every utterance slot b has its own
 * counter in the state (three int32 words per slot behind the caches: chunks decoded, status, output frames decoded; all
 * earlier bytes of the state keep their offsets, and m3_engine_stream_state_size covers them).
 * m3_engine_forward_chunk_slots: one chunk for every slot that is LIVE in this call, i.e. whose chunk_feat_len[b] yields at
 *   least one output frame (pass 0 for fewer than 7 feature frames, as above).  Slot b's window is the one that starts
 *   at ITS input frame 4 c (chunks slot b has decoded).  An idle slot (chunk_feat_len[b] = 0) keeps its counter, K / V history and conv cache
 *   exactly as they were, so a stream may pause for any number of calls; its logits rows are undefined.  A slot whose chunk
 *   would end past max_frames is treated as idle by every kernel (no address is formed from its counter) and its status
 *   word is set until the slot is restarted.  Which slots are live is device data: every call replays the same hipGraph.
 *   The binding is separate from the lockstep binding of the same buffers (same stage names; "stream.advance" is per slot).
 * m3_engine_stream_reset_slots: restarts the n slots listed in `slots` (device int32[n], entries outside [0, B) skipped)
 *   in one launch: counter 0, status cleared, both halves of every block's conv cache refilled.  The K / V history is not
 *   cleared: no kernel reads a position the slot's current stream has not written.
 * m3_engine_stream_positions: frames[b] (device int32[B]) = output frames slot b has decoded since its restart, -1 for a
 *   slot whose status word is set (the convention of m3_ctc_greedy_stream_tokens).
 * m3_engine_stream_reset initialises the slot words too.  One state is driven in ONE mode between two full resets: the
 * lockstep counter and the slot counters do not follow each other. */
int m3_engine_stream_reset_slots(m3_engine* engine, const m3_stream_desc* desc, void* state, size_t state_bytes,
                                 const int32_t* slots, int n, m3_stream stream);
int m3_engine_forward_chunk_slots(m3_engine* engine, const m3_stream_desc* desc, void* state, size_t state_bytes,
                                  const float* feat_chunk, const int32_t* chunk_feat_len, float* logits, void* workspace,
                                  size_t workspace_bytes, int use_graph, m3_stream stream);
int m3_engine_stream_positions(m3_engine* engine, const m3_stream_desc* desc, const void* state, size_t state_bytes,
                               int32_t* frames, m3_stream stream);
/* Expert parallel: rows per wire chunk for the bindings made from now on (what the ranks agreed on: the largest row
 * count B*T' of any rank, so that a rank may send all of its rows to one peer; 0 = this rank's own row count).  The wire
 * buffers "ep.wire_a" / "ep.wire_b" ([world][1 + rows_per_chunk][D] fp32 each, inside the workspace) are what the host
 * hands to the all-to-all: after "blocks.N.moe_ep.send" exchange wire_a -> wire_b, after "blocks.N.moe_ep.expert" again
 * wire_a -> wire_b, then "blocks.N.moe_ep.combine".  Semantics: trainer_3m_fix/fmoe/functions.py:13-86,175-199. */
int m3_engine_set_ep_capacity(m3_engine* engine, int rows_per_chunk);
int m3_engine_num_stages(const m3_engine* engine);
int m3_engine_num_captures(const m3_engine* engine); /* hipGraphs captured so far (a cache hit replays, it does not capture) */
const char* m3_engine_stage_name(const m3_engine* engine, int index);
int m3_engine_run(m3_engine* engine, int first_stage, int last_stage, m3_stream stream);
/* Device address (inside the bound workspace) and size of a named intermediate of the prepared shape:
 * "x" (residual stream, S*D), "xn" (LayerNorm'd MoE input), "embed", "lens" (B int32),
 * "blocks.N.gate_idx" / "gate_value" / "mapping" / "acc_histogram", "blocks.N.out" (debug_taps only). */
int m3_engine_buffer(const m3_engine* engine, const char* name, void** ptr, size_t* bytes);
int m3_engine_num_kernels(const m3_engine* engine);
/* What a stage of the prepared shape launches, for measurement (bench.py prices each stage against the roofline):
 * `kernel` = the device kernel the stage's dispatcher picks for this shape, `launches` = kernel launches of the stage,
 * `alg_bytes` / `flops` = algorithmic HBM bytes (operands read once, results written once) and FLOPs (2 per MAC) of one
 * run with every padded row live; `per_row` = 1 when both scale with the live rows of a packed ragged batch;
 * alg_bytes < 0: data-dependent (the grouped expert FFN: touched experts x weight bytes, priced by the caller from
 * the routing taps). */
typedef struct m3_stage_info {
  const char* kernel;
  int32_t launches;
  int32_t per_row;
  double alg_bytes;
  double flops;
} m3_stage_info;
int m3_engine_stage_info(const m3_engine* engine, int index, m3_stage_info* info);

/* Audio in: Kaldi-style log-Mel filter bank on the device (csrc/fbank.hip) -- compute-fbank-feats with the
 * options of a served model.  Mono PCM at 16 kHz, int16 or float32 in the int16 value range (no scaling to +-1); frames of
 * 400 samples every 160, snip_edges: m3_fbank_num_frames(n) = 0 for n < 400, else 1 + (n - 400) / 160, frame k reads samples
 * [160 k, 160 k + 400).  Per frame: subtract the mean, pre-emphasis 0.97, Povey window, zero-pad to 512, power spectrum of bins
 * 0..255, num_mel_bins triangles equally spaced on mel(f) = 1127 ln(1 + f / 700) between low_freq and high_freq with weights
 * taken in the mel domain (both edges open), log(max(E, FLT_EPSILON)).  No dither, no energy column, no CMVN.
 * Tables (FFT twiddles, window, mel weights) are built on the HOST in float64 and rounded once to float32; the kernel calls
 * no sincos / pow, so the result does not depend on the device's math library.
 * m3_fbank_tables_bytes: size of the table image, host-only; 0 (and m3_last_error) unless 1 <= num_mel_bins <= 128.
 * m3_fbank_tables_host: builds the image into HOST memory of that size (host-only, needs no device).  sample_rate must be
 *   16000, 0 <= low_freq < high_freq <= sample_rate / 2.
 * m3_fbank_tables_init: builds the same image and uploads it to DEVICE memory `tables` (16-byte aligned) on `stream`; the
 *   upload has finished when the call returns.
 * m3_fbank: ONE launch featurises a ragged batch.  pcm (B, ld_pcm) int16 (pcm_is_int16 != 0) or float32, 16-byte aligned
 *   with a row stride of whole 16 bytes (ld_pcm a multiple of 8 / 4 samples); n_samples [B] int32 (device) = samples of
 *   row b, clamped to [0, ld_pcm].  feat (B, T, ld_feat) float32, ld_feat >= num_mel_bins: frames t < feat_len[b] hold the
 *   features, frames feat_len[b] <= t < T are written as ZEROS, columns >= num_mel_bins are not touched.  feat_len_out [B]
 *   int32 (device) = min(m3_fbank_num_frames(n_samples[b]), T).  A frame's result depends on its 400 samples only (not on B,
 *   T, its place in the batch or on which other frames are live) and is the same bits for int16 and float32 input. */
size_t m3_fbank_tables_bytes(int num_mel_bins);
int m3_fbank_tables_host(int num_mel_bins, float sample_rate, float low_freq, float high_freq, void* host_tables);
int m3_fbank_tables_init(int num_mel_bins, float sample_rate, float low_freq, float high_freq, void* tables, m3_stream stream);
int m3_fbank_num_frames(int n_samples);
int m3_fbank(const void* tables, const void* pcm, int pcm_is_int16, int ld_pcm, const int32_t* n_samples, int B, int T,
             int num_mel_bins, float* feat, int ld_feat, int32_t* feat_len_out, m3_stream stream);

/* Delta features in: Kaldi's DeltaFeatures (add-deltas, feat/feature-functions.cc) on the device (csrc/deltas.hip, DESIGN.md
 * 32): static frames -> static | delta | delta-delta, the columns a model trained with the loader's add_deltas reads.
 * scales_0 = [1], scales_i = conv(scales_{i-1}, [-W..W]) / sum_j j^2 (2 i W + 1 taps); block i of output frame t of row b is
 *     sum_{j = -iW..iW} scales_i[j] x[clamp(lead[b] + t + j, 0, n_in[b] - 1)]
 * -- the clamp is on the COMPOSITE filter's taps on the static frames (Kaldi's edge replication; iterating a first-order delta
 * with replicate padding gives other values in the first and last W frames).  order in {1, 2}, window W in [1, 4], so the
 * context is R = order * W <= M3_DELTAS_MAX_CONTEXT frames; anything else is refused.  Tables are built on the HOST in float64
 * and rounded once to float32.
 * m3_deltas_tables_host: host-only, needs no device.  scales: (order + 1) rows of 2 * M3_DELTAS_MAX_CONTEXT + 1 floats, row i
 *   holds scales_i[j] at column M3_DELTAS_MAX_CONTEXT + j and zeros elsewhere.
 * m3_add_deltas: ONE launch for a ragged batch.  feat (B, T_in, ld_feat) float32 with row stride ld_feat >= bins and batch
 *   stride batch_stride_feat (floats), 1 <= bins <= 256.  Device vectors of B int32: n_in = static frames present (clamped to
 *   [0, T_in]); lead (nullable = 0) = frames in front that are context only (clamped to [0, n_in]); n_out = frames to
 *   produce, clipped to n_in - lead and to T_out.  Output frame t is the filter centred on input frame lead + t: offline is
 *   lead = 0, n_out = n_in; in a streaming window real history and lookahead are used where the window holds them, and where
 *   it starts or ends at the utterance's edge the clamp is Kaldi's.  out (B, T_out, ld_out) float32, ld_out >= (order + 1) *
 *   bins, batch stride batch_stride_out: columns [0, bins) get the static frame bit for bit, [i bins, (i + 1) bins) block i;
 *   frames t >= n_out[b] are written as ZEROS; columns >= (order + 1) * bins are not touched.  out_len (nullable) [B] int32
 *   receives the clipped n_out.  IN-PLACE form: out == feat with equal strides and lead == NULL leaves the static columns
 *   alone and writes the delta columns only (m3_fbank writes an engine input buffer, this fills in beside it); any other
 *   overlap of out and feat is the caller's error, out == feat otherwise is refused.  16-byte accesses are used when bins,
 *   all four strides and both pointers are multiples of 4 floats.  Each value is one fp32 fma chain from 0 over its taps in
 *   ascending j and depends on its taps and the table only -- not on B, T_out, lead or which path ran -- so a stream computed
 *   window by window equals the utterance computed at once.  B == 0 or T_out == 0 launches nothing. */
#define M3_DELTAS_MAX_CONTEXT 8
int m3_deltas_tables_host(int order, int window, float* scales);
int m3_add_deltas(const float* feat, int ld_feat, int64_t batch_stride_feat, int T_in, const int32_t* n_in, const int32_t* lead,
                  const int32_t* n_out, int B, int T_out, int bins, int order, int window, float* out, int ld_out,
                  int64_t batch_stride_out, int32_t* out_len, m3_stream stream);

/* Audio in at any sample rate: Kaldi's LinearResample on the device (csrc/resample.hip) -- what
 * compute-fbank-feats does (ResampleWaveform) when a wave's rate is not the feature rate.  With ri = rate_in, ro = rate_out,
 * g = gcd(ri, ro), in_unit = ri / g, out_unit = ro / g, cutoff = 0.99 * 0.5 * min(ri, ro), Z = 6, ww = Z / (2 cutoff): output o
 * has phase p = o % out_unit and unit u = o / out_unit and is
 *     y[o] = sum_{j < n[p]} w[p][j] * x[first[p] + u * in_unit + j],         x = 0 outside the signal,
 * with, for t = p / ro: first[p] = ceil((t - ww) ri), n[p] = floor((t + ww) ri) - first[p] + 1,
 * w[p][j] = window(dt) filt(dt) / ri at dt = (first[p] + j) / ri - t, window(dt) = 0.5 (1 + cos(2 pi cutoff / Z dt)) for
 * |dt| < ww, else 0, filt(dt) = sin(2 pi cutoff dt) / (pi dt), 2 cutoff at dt = 0.  Two deliberate departures: ri == ro is the
 * IDENTITY (one phase, one tap of 1.0; the feature pipeline does not resample then), and interleaved channels are reduced on
 * the way in: the mono sample is (x_0 + ... + x_{C-1}) / (float)C, summed in fp32 in channel order, or channel k alone.
 * Arithmetic: the tables are built on the HOST in float64 and every weight is rounded once to float32; an output is one fp32
 * accumulator from 0, its taps in ascending j, multiply then add (never fused); it is float32, neither rounded nor clamped to
 * int16 (m3_fbank reads it as it is).  An output's bits depend on its absolute index o, its tap inputs and the table only:
 * not on B, the row, where a launch's window starts, or on int16 against float32 input.  So a stream resampled piece by
 * piece equals the whole resampled at once.
 * m3_resample_tables_bytes: size of the table image, host-only; 0 (and m3_last_error) when the pair is refused: a rate outside
 *   [1000, 384000], more than 512 taps per output (max_taps), or more than 2^20 weights (out_unit * max_taps).
 * m3_resample_tables_host: builds the image into HOST memory of that size (host-only, needs no device).  Image: int32
 *   rate_in, rate_out, in_unit, out_unit, max_taps, w_offset (of the weights, in 4-byte words), 2 reserved; int32
 *   first[out_unit], n[out_unit], padded to 16 bytes; float w[max_taps][out_unit] (phase-minor, zero where j >= n[p]).
 * m3_resample_tables_init: builds the same image and uploads it to DEVICE memory `tables` (16-byte aligned) on `stream`; the
 *   upload has finished when the call returns.
 * m3_resample_num_samples: outputs that n_in input samples admit (host-only; -1 on bad rates).  tick = lcm(ri, ro),
 *   L = n_in * (tick / ri), without flush L -= floor(ww * tick); 0 if L <= 0, else last = L / (tick / ro), one less if that
 *   divides exactly, count = last + 1.  flush != 0: the stream has ended and the missing future is zeros.  Without flush no
 *   admitted output reads an input at or beyond n_in.  ri == ro: n_in.
 * m3_resample_input_span: the half-open range [first_in, end_in) of absolute input indices that outputs
 *   [out0, out0 + n_out) read (host-only); first_in may be negative; empty (end_in = first_in) for n_out <= 0.
 * m3_resample: ONE launch resamples a ragged batch.  pcm (B, ld_pcm) int16 (pcm_is_int16 != 0) or float32, `channels` in
 *   [1, 8] interleaved, 16-byte aligned with a row stride of whole 16 bytes (ld_pcm, in elements, a multiple of 8 / 4);
 *   channel = -1: the mean of all channels, k in [0, channels): channel k alone.  Per row b (device vectors): in0[b] int64 =
 *   absolute index of the row's first input sample, n_in[b] int32 = samples per channel in the row, clamped to
 *   [0, ld_pcm / channels]; input outside [in0, in0 + n_in) reads as 0; out0[b] int64 >= 0 = absolute index of the first
 *   output, n_out[b] int32 = outputs wanted, clamped to [0, N_out].  out (B, ld_out) float32, 16-byte aligned, ld_out >= N_out:
 *   out[b][i] = y[out0[b] + i] for i < n_out[b], columns n_out[b] <= i < N_out are written as ZEROS, columns >= N_out are not
 *   touched.  All index arithmetic on absolute positions is 64-bit. */
size_t m3_resample_tables_bytes(int rate_in, int rate_out);
int m3_resample_tables_host(int rate_in, int rate_out, void* host_tables);
int m3_resample_tables_init(int rate_in, int rate_out, void* tables, m3_stream stream);
int64_t m3_resample_num_samples(int rate_in, int rate_out, int64_t n_in, int flush);
int m3_resample_input_span(int rate_in, int rate_out, int64_t out0, int64_t n_out, int64_t* first_in, int64_t* end_in);
int m3_resample(const void* tables, const void* pcm, int pcm_is_int16, int channels, int channel, int ld_pcm, const int64_t* in0,
                const int32_t* n_in, const int64_t* out0, const int32_t* n_out, int B, int N_out, float* out, int ld_out,
                m3_stream stream);

/* Long recordings in: energy VAD, a segmenter and the cut of feature rows into an engine batch (csrc/vad.hip)
 * -- what a Kaldi-style pipeline puts between the features and the decoder (compute-vad, a segmenter, batching), so that a
 * full-context model whose positional table ends at max_len can be run on a recording of any length.  Four launches, all
 * on ragged batches with device length vectors; no result depends on B, T or the launch geometry; all options travel by
 * value; B == 0 or T == 0 (gather: T_max == 0) launches nothing.
 * m3_vad_log_energy: Kaldi's raw frame energy with the framing of m3_fbank (400 samples every 160, snip_edges), so frame k
 *   here is frame k of the features.  Per frame: mean = (sum x) / 400, E = sum (x - mean)^2, log(max(E, FLT_EPSILON)) -- after
 *   DC removal, before pre-emphasis and window.  pcm (B, ld_pcm) int16 (pcm_is_int16 != 0) or float32 in the int16 range, with
 *   the alignment rules of m3_fbank (16-byte aligned, ld_pcm a multiple of 8 / 4 samples); n_samples [B] int32 (device),
 *   clamped to [0, ld_pcm].  log_energy (B, ld_out >= T) float32: frames t < len_out[b] hold the value, frames len_out[b] <= t
 *   < T are written as ZEROS, columns >= T are not touched.  len_out [B] int32 = min(m3_fbank_num_frames(n_samples[b]), T).
 *   Both sums are fp32 in one fixed lane order, so int16 and float32 input give the same bits.
 * m3_vad_decide: Kaldi's ComputeVadEnergy on a log-energy matrix (B, ld_e >= T), lens [B] int32 (device, clamped to [0, T]).
 *   threshold_b = (float)(energy_threshold + energy_mean_scale * mean_b), mean_b = the float64 mean of the fp32 values
 *   logE[b][t < lens[b]] (0 for an empty row), the expression evaluated in float64 and rounded once.  Frame t is voiced iff
 *   (float)num >= (float)den * proportion_threshold (fp32, as Kaldi), den = frames of [t - context, t + context] inside
 *   [0, lens[b]), num = those of them with logE > threshold_b.  flags (B, ld_flags >= T) uint8: 1 / 0, ZEROS for lens[b] <= t <
 *   T, columns >= T not touched; threshold_out [B] float32.  Refused unless 0 <= context <= M3_VAD_MAX_CONTEXT, 0 <
 *   proportion_threshold < 1, energy_mean_scale >= 0.  Kaldi's defaults are 5.0, 0.5, 0, 0.6.
 * m3_vad_segments: flags + log-energy -> the sorted segment list of every row.  Options in frames; refused unless
 *   min_silence >= 0, pad >= 0, min_speech >= 7, 2 pad <= min_silence, 1 <= split_search <= max_segment - 7.  Applied in this
 *   order: CLOSE a silence run strictly between two voiced runs and shorter than min_silence becomes voiced; OPEN a voiced
 *   run shorter than min_speech is dropped; PAD run [s, e) becomes [max(s - pad, 0), min(e + pad, len)) (runs cannot touch,
 *   by 2 pad <= min_silence); SPLIT while a run is longer than max_segment it is cut at the frame of lowest logE in
 *   [s + max_segment - split_search, s + max_segment), the lowest index on a tie; [s, cut) is emitted and the rest goes on
 *   from cut.  A flag counts only for t < lens[b].  segments (B, capacity, 2) int32 [start, end), ascending; n_segments [B]
 *   int32 = the TRUE count even when it exceeds capacity: only the first `capacity` are written and nothing behind them (the
 *   overflow report of the bounded EP wire).  A row is streamed by one wave, whatever its length.
 * m3_segment_gather: cuts rows of ONE long feature matrix src (T_all, ld_src >= cols) float32 into an engine batch.  jobs
 *   [B][3] int32 (device) = (src_row, start, end): segment b is rows src_row + [start, end) of src.  dst (B, T_max, ld_dst >=
 *   cols) with batch stride batch_stride_dst: frame t < n_b = min(end - start, T_max) gets its row bit for bit in columns
 *   [0, cols), frames n_b <= t < T_max are written as ZEROS, columns >= cols are not touched; len_out [B] int32 = n_b.  A job
 *   that leaves [0, T_all) is cut short where it leaves (to nothing if it starts outside) and reports the shortened count.
 *   16-byte accesses when cols, the three strides and both pointers are multiples of 4 floats.  Features are computed once
 *   over the whole recording and THEN cut, so the delta columns at a segment's edges come from the real neighbouring frames,
 *   not from a replicated edge: the deliberate difference from featurising cut audio. */
#define M3_VAD_MAX_CONTEXT 32
int m3_vad_log_energy(const void* pcm, int pcm_is_int16, int ld_pcm, const int32_t* n_samples, int B, int T, float* log_energy,
                      int ld_out, int32_t* len_out, m3_stream stream);
int m3_vad_decide(const float* log_energy, int ld_e, const int32_t* lens, int B, int T, float energy_threshold,
                  float energy_mean_scale, int context, float proportion_threshold, uint8_t* flags, int ld_flags,
                  float* threshold_out, m3_stream stream);
int m3_vad_segments(const uint8_t* flags, int ld_flags, const float* log_energy, int ld_e, const int32_t* lens, int B, int T,
                    int min_silence, int min_speech, int pad, int max_segment, int split_search, int32_t* segments,
                    int capacity, int32_t* n_segments, m3_stream stream);
int m3_segment_gather(const float* src, int ld_src, int T_all, const int32_t* jobs, int B, int T_max, int cols, float* dst,
                      int ld_dst, int64_t batch_stride_dst, int32_t* len_out, m3_stream stream);

/* Attention rescoring: the AED decoder's second pass over the CTC n-best (csrc/aed_rescore.hip).  The decoder
 * runs teacher-forced on PACKED hypothesis rows: hypothesis slot h = b * beam + i owns rows [hyp_row0[h], hyp_row0[h + 1]) of
 * every row buffer, len + 1 of them for a live slot (sos, then its tokens) and none for a slot i >= n_hyps[b] (n_hyps < 0, a
 * failed search, counts as 0).  The dense layers between these kernels are m3_linear calls.  All kernels are fp32 and
 * deterministic: no atomics, every reduction in a fixed order, a row's result independent of where the row lies.  All
 * pointers are device memory.
 * m3_aed_embed: decoder input x [rows][ldx] = emb[tok] * sqrt(D) + pe[pos] for the input tokens (sos, y_0 .. y_{n-1}), or
 *   (sos, y_{n-1} .. y_0) with reverse != 0, and target [rows] = the token each row has to predict (the input shifted by one,
 *   then eos = sos).  hyp_tokens [B][beam][max_frames] / hyp_len / n_hyps as m3_ctc_beam_*_nbest leave them; hyp_row0
 *   [B * beam + 1].  emb [V][D], pe [pe_rows][D].  A slot whose row range disagrees with its length, leaves [0, rows) or
 *   needs more than pe_rows positions is skipped; a token outside [0, V) gives a row of NaN.  D a multiple of 4, ldx >= D.
 * m3_aed_attention: multi-head attention core on packed query rows, online softmax over key tiles staged in LDS, no score
 *   matrix in memory.  att_desc [n_slots][5] int32 = (q_row0, n_q, kv_row0, kv_len, causal) per hypothesis slot: its n_q
 *   query rows start at row q_row0 of q / out, its keys and values are rows [kv_row0, kv_row0 + kv_len) of k / v; causal:
 *   query i sees keys j <= i.  Self-attention points a slot at its own rows (causal = 1), source attention at the memory
 *   rows of its utterance, which the whole beam shares.  q [q_rows][ldq], k [kv_rows][ldk], v [kv_rows][ldv], out
 *   [q_rows][ldo], head h in columns [h dk, (h + 1) dk).  max_q >= every n_q (sizes the grid).  dk a multiple of 16, <= 128;
 *   ldq / ldk / ldv multiples of 4 and the pointers 16-byte aligned.  A slot with n_q <= 0 does nothing; a slot with
 *   kv_len <= 0 or a range outside [0, q_rows) / [0, kv_rows) is skipped (its rows stay unwritten): the caller rejects
 *   kv_len = 0 before it builds the descriptors.
 * m3_aed_score: per packed row logsumexp over V and the target's logit (one wave per row), per hypothesis their sum in row
 *   order, att [B][beam]; with r_logits the same for the right-to-left decoder, r_att; final = (1 - reverse_weight) att +
 *   reverse_weight r_att + ctc_weight prior (the r_att term only with r_logits, the prior term only with ctc_weight != 0);
 *   best [B] = the first slot with the strictly largest final, -1 for an utterance without hypotheses.  Dead slots report
 *   -inf in att / r_att / final (r_att is 0 for live slots without r_logits).  logits [rows][ldl], r_logits NULL or
 *   [rows][ldrl], target / r_target [rows], prior [B][beam] (may be NULL when ctc_weight = 0), row_logp [2 * rows] scratch.
 *   1 <= beam <= 64. */
int m3_aed_embed(const int32_t* hyp_tokens, const int32_t* hyp_len, const int32_t* n_hyps, const int32_t* hyp_row0, int B,
                 int beam, int max_frames, const float* emb, const float* pe, int pe_rows, int V, int D, int reverse, int rows,
                 float* x, int ldx, int32_t* target, m3_stream stream);
int m3_aed_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* att_desc,
                     int n_slots, int max_q, int q_rows, int kv_rows, int H, int dk, float scale, float* out, int ldo,
                     m3_stream stream);
int m3_aed_score(const float* logits, int ldl, const float* r_logits, int ldrl, const int32_t* target, const int32_t* r_target,
                 const int32_t* hyp_row0, const int32_t* n_hyps, const float* prior, int B, int beam, int rows, int V,
                 float ctc_weight, float reverse_weight, float* row_logp, float* att, float* r_att, float* final_score,
                 int32_t* best, m3_stream stream);

/* Streaming two-pass decoding: the encoder memory of B live streams, kept per slot on the device so that a stream's n-best can
 * be rescored when its utterance ends (csrc/aed_memory.hip).  One state blob per streaming decoder, caller-owned
 * device memory of m3_aed_memory_state_size bytes (16-byte aligned; 0 and m3_last_error for a descriptor the library
 * rejects: D a multiple of 4, B and max_frames >= 0).  Per slot it holds max_frames rows of D fp32 and two words, the rows
 * held (len) and a status.  The rows are COPIES of the residual stream before after_norm (the chunk binding's buffer "x"):
 * the rescorer applies after_norm in the prologue of its K / V GEMM, so nothing is normalised here.  All calls of one state
 * are enqueued on one stream; none synchronises with the host.  Row loads and stores are 16 bytes wide, there are no atomics.
 * BOUNDARY RULE: the memory of an utterance is exactly the frames its n-best was searched over -- the caller appends with
 * the same n_frames the beam search advances by, the frames of an endpoint's firing chunk behind the endpoint included.
 * m3_aed_memory_reset / _reset_slots: len = 0, status cleared, for all B slots or for the n slots listed in `slots` (device
 *   int32[n], entries outside [0, B) skipped).  Only the words are cleared: no kernel reads a row the slot's current stream
 *   has not written.
 * m3_aed_memory_append: x [B * T_chunk][ldx], rows b * T_chunk + t with t < clamp(n_frames[b], 0, T_chunk) go to positions
 *   len[b] + t of slot b, then len[b] moves (n_frames [B] int32 on the device).  A slot with 0 frames keeps its words and rows
 *   exactly as they are.  A slot that would pass max_frames consumes nothing and its status is set until the slot is reset
 *   (the convention of m3_ctc_greedy_stream_advance).  One work-group per slot reads the words once, copies, passes a barrier
 *   and then moves the length.  ldx >= D and a multiple of 4, x 16-byte aligned, T_chunk <= 2^14.
 * m3_aed_memory_lengths: len [B] = rows slot b holds, -1 for a slot whose status is set.
 * m3_aed_memory_gather: the valid rows of the n slots listed in `slots` (device int32[n], n <= 65535) packed one after the
 *   other in list order into out [out_rows][ldo]; out_row0 [n + 1] = the prefix sums of their lengths.  A failed slot and an
 *   entry outside [0, B) contribute 0 rows.  Rows at or past out_rows are not written (out_row0 still tells the full sums, so
 *   n * max_frames rows always suffice); rows past out_row0[n] are not touched.  ldo >= D and a multiple of 4, out 16-byte
 *   aligned. */
typedef struct m3_aed_memory_desc {
  int32_t B;
  int32_t max_frames;
  int32_t D;
} m3_aed_memory_desc;
size_t m3_aed_memory_state_size(const m3_aed_memory_desc* desc);
int m3_aed_memory_reset(const m3_aed_memory_desc* desc, void* state, size_t state_bytes, m3_stream stream);
int m3_aed_memory_reset_slots(const m3_aed_memory_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n,
                              m3_stream stream);
int m3_aed_memory_append(const m3_aed_memory_desc* desc, void* state, size_t state_bytes, const float* x, int ldx, int T_chunk,
                         const int32_t* n_frames, m3_stream stream);
int m3_aed_memory_lengths(const m3_aed_memory_desc* desc, const void* state, size_t state_bytes, int32_t* len, m3_stream stream);
int m3_aed_memory_gather(const m3_aed_memory_desc* desc, const void* state, size_t state_bytes, const int32_t* slots, int n,
                         float* out, int ldo, int out_rows, int32_t* out_row0, m3_stream stream);

/* Attention decoding: the AED decoder's own autoregressive beam search (csrc/aed_search.hip).  R = B * beam
 * hypothesis rows, row r = u * beam + slot; one new token per row per step; sos = eos = V - 1.  Everything that changes from
 * step to step lives in the state blob, so a step is the same launches with the same arguments every time and the host reads
 * nothing to issue the next one:  m3_aed_search_embed, then per decoder layer [m3_linear qkv (norm1 prologue),
 * m3_aed_search_attention (self), m3_linear out (+ residual), m3_linear q (norm2), m3_aed_search_attention (source), m3_linear
 * out (+ residual), m3_linear w_1 (norm3, activation), m3_linear w_2 (+ residual)], m3_linear output layer (after_norm),
 * m3_aed_search_prune.  fp32, no atomics, fixed reduction orders, a row's result independent of its place in the batch.
 * State blob: caller-owned device memory of m3_aed_search_state_size bytes, 16-byte aligned (0 and m3_last_error for a
 *   descriptor the library rejects: 1 <= beam <= min(64, V), max_steps >= 1, D / H a multiple of 16 up to 128, sizes that
 *   overflow the int32 row arithmetic).  Per utterance: its own step counter, its limit, a done flag and its memory rows.
 *   Per row, double-buffered by the parity of the utterance's step: score, finished flag, the token path [max_steps + 1]
 *   (position 0 = sos) and the ancestry path[t] = the slot that wrote position t of the hypothesis's self-attention keys.
 * K / V cache: caller-owned, m3_aed_search_cache_size bytes = layers * max_steps * R * 2 D fp32, laid out
 *   [layer][position][R][K (D) | V (D)]; written once per (position, slot), never moved: pruning copies the integer paths.
 * m3_aed_search_reset: every row holds [sos]; slot 0 scores 0, the others -inf; utterance u owns memory rows
 *   [mem_row0[u], mem_row0[u] + mem_len[u]) (device int32 [B]) and stops after limit = min(mem_len, pe_rows - 1, max_steps)
 *   steps (max_steps <= desc->max_steps); mem_len < 1 marks it done at once (the caller refuses that before it launches).
 * m3_aed_search_embed: x [R][ldx] = emb[last token of r] * sqrt(D) + pe[step of r's utterance].  emb [V][D], pe [pe_rows][D].
 * m3_aed_search_attention: single-query attention, one wave per (row, head), online softmax over tiles of 64 keys.
 *   cache != NULL, self use: kv [R][ldkv] holds the rows' new K | V (columns [0, D) and [D, 2 D): the fused QKV GEMM's output
 *   from column D on); the wave stores its head's slice at cache position `step` under the row's own slot, then attends over
 *   positions 0 .. step, position t < step fetched from slot path[t], the last one from kv itself.  cache == NULL, source use:
 *   kv [kv_rows][ldkv] = the memory's K | V projection of `layer` (columns as above), keys = the utterance's memory rows, shared
 *   by its beam.  q [R][ldq], out [R][ldo], head h in columns [h dk, (h + 1) dk); ldkv a multiple of 4, kv / cache 16-byte
 *   aligned.  Rows of a done utterance are skipped (nothing stored, out untouched).
 * m3_aed_search_prune: one work-group per utterance: per row logsumexp over V and the beam largest logits (lower token id on
 *   ties), a finished row offering the single candidate (increment 0, eos) instead; the beam largest of the beam^2 candidate
 *   scores (lower flat index slot * beam + rank on ties; a candidate of a -inf slot stays -inf); new tokens, scores, flags
 *   and ancestry go to the other record;  a NaN is never picked, neither as a logit nor as a candidate score: a row holding a
 *   NaN logit has a NaN logsumexp and so offers no candidate, a rank of a row without a logit left is (-inf, eos), and a new
 *   slot without a candidate left is (-inf, eos) under parent 0; the utterance's step moves and its done flag is set once every slot is finished or
 *   the limit is reached.  A done utterance is left bit for bit alone.  logits [R][ldl]; done: NULL or device int32 [B] that
 *   receives every utterance's done flag (the one word the host polls).
 * m3_aed_search_result: hyp_tokens [B][beam][max_steps] (sos and trailing eos stripped, -1 behind), hyp_len, score, finished
 *   [B][beam], best [B] = the first slot with the strictly largest score, steps [B] = steps taken. */
typedef struct m3_aed_search_desc {
  int32_t B;
  int32_t beam;
  int32_t max_steps;
  int32_t V;
  int32_t D;
  int32_t H;
  int32_t layers;
  int32_t pe_rows;
} m3_aed_search_desc;
size_t m3_aed_search_state_size(const m3_aed_search_desc* desc);
size_t m3_aed_search_cache_size(const m3_aed_search_desc* desc);
int m3_aed_search_reset(const m3_aed_search_desc* desc, void* state, size_t state_bytes, const int32_t* mem_row0,
                        const int32_t* mem_len, int max_steps, m3_stream stream);
int m3_aed_search_embed(const m3_aed_search_desc* desc, const void* state, size_t state_bytes, const float* emb, const float* pe,
                        float* x, int ldx, m3_stream stream);
int m3_aed_search_attention(const m3_aed_search_desc* desc, const void* state, size_t state_bytes, const float* q, int ldq,
                            const float* kv, int ldkv, int kv_rows, float* cache, size_t cache_bytes, int layer, float* out, int ldo,
                            m3_stream stream);
int m3_aed_search_prune(const m3_aed_search_desc* desc, void* state, size_t state_bytes, const float* logits, int ldl,
                        int32_t* done, m3_stream stream);
int m3_aed_search_result(const m3_aed_search_desc* desc, const void* state, size_t state_bytes, int32_t* hyp_tokens, int32_t* hyp_len,
                         float* score, int32_t* finished, int32_t* best, int32_t* steps, m3_stream stream);

/* Joint CTC/attention decoding (csrc/aed_joint.hip): the search above with every candidate also scored by its CTC
 * prefix probability (Watanabe et al. 2017) and ranked by key = (1 - ctc_weight) att + ctc_weight ctc.  The step is the one
 * above up to the output layer; m3_aed_joint_score and m3_aed_joint_prune then stand where m3_aed_search_prune stood (8 L + 4
 * launches).  The search state, its descriptor and the other m3_aed_search_* calls are used unchanged; a record's score word
 * holds the key, so m3_aed_search_result keeps working.  blank = 0, sos = eos = V - 1 (V >= 2).
 * ctc [ctc_rows][ldc]: natural-log CTC probabilities over the same V, one row per memory row: utterance u reads rows
 *   [mem_row0[u], mem_row0[u] + mem_len[u]) as the search state's headers name them.  An utterance whose rows do not lie
 *   inside [0, ctc_rows) or exceed max_frames is read nowhere: all its CTC parts are -inf (the caller refuses it before).
 * Scorer state: caller-owned, m3_aed_joint_state_size bytes, 16-byte aligned; per row, double-buffered by the parity of the
 *   utterance's step: att, ctc (the two parts of the key), and the prefix scorer's rn / rb over max_frames frames.
 * Scratch: caller-owned, m3_aed_joint_scratch_size bytes, 16-byte aligned; rewritten by every step: beam * pre_beam candidate
 *   records per utterance and every candidate's extended rn / rb, from which prune copies the survivors' (it recomputes nothing).
 * m3_aed_joint_reset: after m3_aed_search_reset on the same stream.  The empty hypothesis's state in every slot: rn = -inf,
 *   rb[t] = the running sum of ctc[.][0], ctc part 0; att part 0 in slot 0, -inf in the others.
 * m3_aed_joint_score: one wave per row: logsumexp of logits [R][ldl] and the pre_beam largest (m3_aed_search_prune's pick order),
 *   candidate j's recursion over the frames in lane j; a finished row offers (eos, its parts unchanged) alone.
 *   0 < ctc_weight <= 1.  A part at -inf makes the key -inf.
 * m3_aed_joint_prune: one work-group per utterance: the beam largest keys (lower flat index slot * pre_beam + rank on ties),
 *   paths, flags, step and done exactly as m3_aed_search_prune; parts and scorer states go to the other buffer.
 * m3_aed_joint_result: att, ctc [B][beam], the parts of the hypotheses m3_aed_search_result returns. */
typedef struct m3_aed_joint_desc {
  m3_aed_search_desc search;
  int32_t pre_beam;    /* beam <= pre_beam <= min(64, V) */
  int32_t max_frames;  /* the most memory frames of an utterance */
} m3_aed_joint_desc;
size_t m3_aed_joint_state_size(const m3_aed_joint_desc* desc);
size_t m3_aed_joint_scratch_size(const m3_aed_joint_desc* desc);
int m3_aed_joint_reset(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, void* joint_state,
                       size_t joint_state_bytes, const float* ctc, int ldc, int ctc_rows, m3_stream stream);
int m3_aed_joint_score(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                       size_t joint_state_bytes, void* scratch, size_t scratch_bytes, const float* logits, int ldl, const float* ctc,
                       int ldc, int ctc_rows, float ctc_weight, m3_stream stream);
int m3_aed_joint_prune(const m3_aed_joint_desc* desc, void* search_state, size_t search_state_bytes, void* joint_state,
                       size_t joint_state_bytes, const void* scratch, size_t scratch_bytes, int32_t* done, m3_stream stream);
int m3_aed_joint_result(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                        size_t joint_state_bytes, float* att, float* ctc, m3_stream stream);

/* N-gram LM fusion and a length bonus in that search (csrc/aed_joint.hip): every candidate also takes one step
 * through the LM image above ("LM image"; the score contract of the CTC search's fusion, unchanged) and is ranked by
 *   key = jkey + (float)(alpha * lm + beta * n),   jkey = (1 - ctc_weight) att + ctc_weight ctc,
 * lm the double sum of the LM's log-probabilities over the hypothesis's tokens (eos adds final[state] when use_eos), n its
 * tokens after sos, eos included; the two products and the sum in double, rounded once.  A -inf jkey stays -inf.  The score
 * and prune calls below stand where the joint ones stood, so the step keeps its 8 L + 4 launches.  ctc_weight = 0 is legal
 * here: the search is then attention plus LM, jkey = att, the ctc part is 0, no CTC input is taken and neither the scorer state
 * nor the joint scratch nor max_frames is looked at (pass NULL / 0); a row still offers pre_beam candidates.
 * An utterance whose lm_on is 0 adds nothing: its records, keys, parts and scorer state are the joint search's, bit for bit.
 * LM state: caller-owned, the first size query's bytes, 16-byte aligned; per row, double-buffered by the parity of the
 *   utterance's step: lm_state, n, lm (double), and the att part where there is no scorer state to hold it.
 * LM scratch: caller-owned, the second size query's bytes, 16-byte aligned; rewritten by every step: every candidate's
 *   (lm_state, lm), from which prune copies the survivors' (nothing is walked twice), and the candidate records when
 *   ctc_weight = 0.  Both sizes depend on B, beam and pre_beam only.
 * reset: after the search's (and the joint search's) reset, once per search.  Reads the image's header back (a synchronous
 *   20-word copy: call it outside a stream capture) and refuses an image that is not one or was built for another V; every
 *   slot then holds the image's start state, lm = 0.0, n = 0.
 * reset_set: reset for an LM set ("LM set" above; a single image is taken too): lm_on (device int32 [B], the values the score
 *   calls of this search will get) picks each utterance's member, and its slots hold THAT member's start state; an utterance
 *   that runs without the LM holds state 0.  Reads the header back like reset and refuses a set built for another V.
 * score: the joint score call plus the walk.  ctc is NULL exactly when ctc_weight == 0.  lm_image / lm_bytes: the DEVICE
 *   image; lm_on: device int32 [B]; alpha, beta finite; use_eos 0 or 1.  The kernel range-checks every word of the image it
 *   forms an address from (a bad state or next state means state 0, a bad arc range "no arcs", a token outside [0, V) unk_logp).
 * prune: the joint prune call plus the survivors' LM state; joint_state is NULL exactly when the search runs without CTC.
 * result: lm [B][beam] (the float32 rounding of the double) and lm_state of the hypotheses the search's result call returns;
 *   n and att (NULL or [B][beam]): the token counts, and the attention parts as the LM state holds them for ctc_weight = 0. */
size_t m3_aed_ngram_state_size(const m3_aed_joint_desc* desc);
size_t m3_aed_ngram_scratch_size(const m3_aed_joint_desc* desc);
int m3_aed_ngram_reset(const m3_aed_joint_desc* desc, void* lm_state, size_t lm_state_bytes, const void* lm_image, size_t lm_bytes,
                    m3_stream stream);
int m3_aed_ngram_reset_set(const m3_aed_joint_desc* desc, void* lm_state, size_t lm_state_bytes, const void* lm_image, size_t lm_bytes,
                           const int32_t* lm_on, m3_stream stream);
int m3_aed_ngram_score(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                    size_t joint_state_bytes, void* scratch, size_t scratch_bytes, const void* lm_state, size_t lm_state_bytes,
                    void* lm_scratch, size_t lm_scratch_bytes, const float* logits, int ldl, const float* ctc, int ldc, int ctc_rows,
                    float ctc_weight, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha, double beta, int use_eos,
                    m3_stream stream);
int m3_aed_ngram_prune(const m3_aed_joint_desc* desc, void* search_state, size_t search_state_bytes, void* joint_state, size_t joint_state_bytes,
                    const void* scratch, size_t scratch_bytes, void* lm_state, size_t lm_state_bytes, const void* lm_scratch,
                    size_t lm_scratch_bytes, int32_t* done, m3_stream stream);
int m3_aed_ngram_result(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* lm_state,
                     size_t lm_state_bytes, float* lm, int32_t* lm_state_out, int32_t* n, float* att, m3_stream stream);

/* Hotword biasing in that search (csrc/aed_joint.hip): every candidate also takes one arc of its utterance's graph
 * in a context set ("context set" above: the image, its limits and m3_ctc_context_validate are the CTC search's, unchanged) and
 * is ranked by
 *   key = jkey + (float)extra,   extra = (alpha * lm + beta * n) + bonus with an LM, bonus without,
 * in double, rounded once; jkey as above (att when ctc_weight = 0).  A -inf jkey stays -inf.  The graph's own score is the
 * weight: there is no further multiplier.  A hypothesis carries ctx_state (0 for [sos]) and bonus (double, 0.0).  A token c that
 * is not eos adds delta[ctx_state][cls[c]] and moves to next[ctx_state][cls[c]]; eos (V - 1) is never walked: it subtracts
 * pot[ctx_state], the credit of a phrase the hypothesis did not complete, and ends in state 0, so a finished hypothesis's bonus is
 * the context contract's `final`.  A hypothesis cut at the step limit keeps its provisional credit in its key; final is then
 * bonus - pot[ctx_state], which the caller forms from what the result call returns.  A finished slot keeps key, bonus and state.
 * The context scores the PRE-BEAM, like the LM: a row offers its pre_beam largest attention log-probabilities whatever ctc_weight
 * and the LM are, and a hotword token outside them is not rescued.
 * graph_of (device int32 [B]) picks a graph per utterance; -1, a value outside [0, G), an image whose header fails its checks or
 * one built for another V mean "unbiased": that utterance's records, keys, parts, scorer state and LM state are, bit for bit,
 * those of the same search without a context, and its context state stays (0, 0.0).
 * The calls below stand where the joint / ngram score and prune calls stood, so the step keeps its 8 L + 4 launches.  They take
 * what the m3_aed_ngram_* calls take, with two freedoms: lm_image, lm_on, lm_state and lm_scratch are NULL exactly when there is
 * no LM (alpha, beta and use_eos are then not used but must be finite), and ctc, joint_state and scratch are NULL exactly when
 * ctc_weight == 0.  With neither, the context state keeps the att part and the context scratch the candidate records.
 * m3_aed_bias: image / image_bytes: the DEVICE context image; graph_of; state: caller-owned, m3_aed_bias_state_size bytes,
 *   16-byte aligned: per row, double-buffered by the parity of the utterance's step: ctx_state, att, bonus (double); scratch:
 *   caller-owned, m3_aed_bias_scratch_size bytes, 16-byte aligned, rewritten by every step: every candidate's (ctx_state, bonus),
 *   from which prune copies the survivors' (nothing is walked twice), and the candidate records of the form without CTC and LM.
 *   Both sizes depend on B, beam and pre_beam only.
 * reset: after the search's (and the joint and ngram) reset, once per search.  Reads the image's 4-word header back (a
 *   synchronous copy: call it outside a stream capture) and refuses an image that is not a context set or was built for another
 *   V; every slot then holds state 0, bonus 0.0.  The image itself must have passed m3_ctc_context_validate on the host.
 * score: one wave per row; the row's ctx_state is wave-uniform, so all lanes gather cls[token], then one row of delta / next.  The
 *   kernel range-checks every word it forms an address from (a bad state or next entry means state 0, a bad class column 0).
 * prune: the survivors' (ctx_state, bonus) go to the other buffer.  image / graph_of of the record are not read.
 * result: bonus [B][beam] (the float32 rounding of the double) and ctx_state of the hypotheses the search's result call returns;
 *   att (NULL or [B][beam]): the attention parts as the context state holds them for the form without CTC and LM.
 * Every call refuses, before any launch: a bad descriptor, a blob that is too small or misaligned, a NULL mismatch, a weight that
 * is not finite. */
typedef struct m3_aed_bias {
  const void* image;       /* device context image */
  size_t image_bytes;
  const int32_t* graph_of; /* device, [B] */
  void* state;
  size_t state_bytes;
  void* scratch;
  size_t scratch_bytes;
} m3_aed_bias;
size_t m3_aed_bias_state_size(const m3_aed_joint_desc* desc);
size_t m3_aed_bias_scratch_size(const m3_aed_joint_desc* desc);
int m3_aed_bias_reset(const m3_aed_joint_desc* desc, const m3_aed_bias* bias, m3_stream stream);
int m3_aed_bias_score(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const void* joint_state,
                      size_t joint_state_bytes, void* scratch, size_t scratch_bytes, const void* lm_state, size_t lm_state_bytes,
                      void* lm_scratch, size_t lm_scratch_bytes, const float* logits, int ldl, const float* ctc, int ldc, int ctc_rows,
                      float ctc_weight, const void* lm_image, size_t lm_bytes, const int32_t* lm_on, double alpha, double beta, int use_eos,
                      const m3_aed_bias* bias, m3_stream stream);
int m3_aed_bias_prune(const m3_aed_joint_desc* desc, void* search_state, size_t search_state_bytes, void* joint_state, size_t joint_state_bytes,
                      const void* scratch, size_t scratch_bytes, void* lm_state, size_t lm_state_bytes, const void* lm_scratch,
                      size_t lm_scratch_bytes, const m3_aed_bias* bias, int32_t* done, m3_stream stream);
int m3_aed_bias_result(const m3_aed_joint_desc* desc, const void* search_state, size_t search_state_bytes, const m3_aed_bias* bias,
                       float* bonus, int32_t* ctx_state, float* att, m3_stream stream);

/* WFST decoding: CTC token-passing beam search over a compiled graph (TLG) on the device (csrc/ctc_wfst.hip, DESIGN.md 38;
 * restated on the host in tests/wfst_ref.py).  The searches above work on tokens; this one walks a weighted transducer in
 * the tropical semiring -- a lexicon composed with a word-level LM and a CTC token topology -- and returns WORDS.
 *
 * Graph image (m3asr.wfst.DecodingGraph builds it; m3_wfst_validate checks a HOST copy before it is uploaded): 4-byte
 * little-endian words.
 *   header, 20 words: [0] magic "M3FS" (0x5346334D)  [1] version 1  [2] V  [3] n_states  [4] n_arcs  [5] start  [6] n_levels
 *     [7] 0  [8..15] word offsets of the tables below, in that order  [16] words in the image  [17..19] 0
 *   arc_begin[n_states + 1], eps_begin[n_states]: the arcs of state s are [arc_begin[s], arc_begin[s + 1]), the emitting
 *     ones first, its epsilon-input arcs from eps_begin[s]; both groups sorted by (ilabel, dst)
 *   arc_ilabel, arc_olabel, arc_dst (int32), arc_weight (float32) [n_arcs];  final (float32), eps_level (int32) [n_states]
 *   ilabel 0 is epsilon and consumes no frame; ilabel i >= 1 consumes one frame of CTC output id i - 1.  olabel 0 is "no
 *   output", olabel >= 1 a word id.  Weights are float32 costs; final = +inf means "not final"; no weight is -0.0.
 *   eps_level[s] is the length of the longest path of epsilon-input arcs ending in s; n_levels = max eps_level + 1.
 * m3_wfst_validate refuses, naming the first offence: a size that is no multiple of 4 or above 1 GiB, a wrong magic, version, V
 *   or word count, n_states outside [1, 2^26], a table outside the image, arc_begin that is not monotone from 0 to n_arcs,
 *   eps_begin outside its state's arcs, an ilabel outside [0, V] or on the wrong side of eps_begin, unsorted arcs, a negative
 *   olabel, a dst outside [0, n_states), an arc weight that is not finite or is -0.0, a final weight that is NaN, -inf or -0.0,
 *   no final state, a cycle of epsilon-input arcs (a state on it is named), a wrong eps_level, n_levels wrong or above 64.
 *
 * The search is Viterbi token passing with one token per graph state.  All cost arithmetic is float32, every add and multiply
 * rounded on its own (no fused multiply-add).  Per utterance: a cost and a history index per live state, and a pool of history
 * records (prev, olabel, frame); a record is made only when an arc with olabel != 0 wins.
 * Ranking.  Everywhere "min" is the minimum of the 64-bit key (ordered bits of cost) << 32 | arc id: on equal cost the smaller
 *   arc index wins; on the device a 64-bit atomic min per destination state, so nothing depends on thread order.  A candidate
 *   whose cost is not finite is dropped.  Costs are never -0.0: the start cost is +0.0, no weight is -0.0 and a sum rounded to
 *   nearest is -0.0 only when both terms are; the ordered-bits key would tell the two zeros apart, a float comparison does not.
 * Start (reset).  A token on the start state, cost +0.0, no history, no arc; then the epsilon closure (d) with frame 0 and
 *   cutoff 0.0 + beam.
 * Frame t, logp its log-softmax row:
 *   (a) best = the smallest live cost; a token is expandable when cost <= best + beam; if more than max_active are, exactly the
 *       max_active smallest by (cost, state id) stay expandable (a radix select over that key).
 *   (b) for every expandable token (s, c) and emitting arc a of s: cand = (c + w_a) + ((-acoustic_scale) * logp[ilabel_a - 1]),
 *       min into next[dst_a].
 *   (c) best_e = the smallest cost in next, cutoff = best_e + beam; a token above cutoff is dropped (not live).  If next is
 *       empty the search is dead: M3_WFST_DEAD, sticky; the frame and all later ones are no-ops and the result is empty.
 *   (d) for L = 0 .. n_levels - 1: every state of next with eps_level L and cost <= cutoff has its final cost (its epsilon
 *       predecessors have lower levels).  Its history is resolved from its winning arc: the source's history of the frame
 *       before for an emitting winner, of this frame for an epsilon winner; if the winner's olabel != 0 a record
 *       (that history, olabel, t) is appended and becomes the state's history.  Then its epsilon arcs are relaxed:
 *       cand = c + w_a, kept only if finite and <= cutoff, min into next[dst_a].  Every token is expanded once, with its final
 *       cost; there is no iteration to a fixed point.  Record indices may differ from run to run, the sequences they encode not.
 *   After (d) next is the live set (its states with cost <= cutoff).
 * Result.  partial (final = 0): the words of the live token with the smallest (cost, state).  final = 1: the smallest
 *   (cost + final[state], state) over live states whose sum is finite, reached_final = 1; if there is none, the partial with
 *   reached_final = 0.  Per utterance: the words, the frame of each word's record, the cost, reached_final, the status.
 * Capacities fail soft.  token_cap bounds the states touched per frame (dropped ones included; checked after (b) and after every
 *   level of (d)), record_cap the record pool (checked when a closure ends), max_frames the frames between resets (a frame
 *   beyond it is not taken).  Exceeding one sets M3_WFST_TOKEN_CAP / RECORD_CAP / MAX_FRAMES in the sticky status; the utterance
 *   stops advancing until its reset and its result is n_words = -1, cost +inf.  Nothing is written out of bounds.
 *
 * m3_wfst_search_desc: n_states, n_levels and V are the graph's (a graph with other values is refused per utterance with
 *   M3_WFST_BAD_GRAPH); beam > 0 (+inf allowed), max_active >= 1, acoustic_scale finite; V <= 12288 (the row is staged in LDS).
 * state: caller-owned device memory, m3_wfst_search_state_size bytes (0 = bad descriptor), 16-byte aligned; per utterance a
 *   16-word header, two dense state-indexed arrays of 64-bit keys and two of history indices (24 bytes per graph state), two
 *   touched lists [token_cap], n_levels worklists [token_cap], the record pool [3][record_cap].  The dense arrays are cleared
 *   through the touched list, never per frame as a whole; reset clears them whole.
 * reset: slots NULL = all B utterances, else n utterance indices (device int32).  Other utterances' bytes are not touched.
 * advance: logp [B][T_chunk][ld] float32 on the device (ld >= V), n_frames[B] (device) frames of each row that count.  One
 *   work-group of 1024 threads per utterance, all frames in one launch, no host sync.
 * result: words / frames [B][max_words] int32 (-1 padded), n_words / flags (reached_final) / status [B] int32, cost [B] float32,
 *   all on the device.  A word sequence longer than max_words gives n_words = -1 and M3_WFST_WORD_CAP in the returned status.
 * Every call refuses, before any launch: a bad descriptor, a state that is too small or misaligned, a null pointer. */
#define M3_WFST_DEAD 1
#define M3_WFST_TOKEN_CAP 2
#define M3_WFST_RECORD_CAP 4
#define M3_WFST_MAX_FRAMES 8
#define M3_WFST_BAD_GRAPH 16
#define M3_WFST_WORD_CAP 32
typedef struct m3_wfst_search_desc {
  int32_t B, max_frames, token_cap, record_cap, max_active;
  int32_t n_states, n_levels, V;
  float beam, acoustic_scale;
} m3_wfst_search_desc;
int m3_wfst_validate(const void* image, size_t image_bytes, int V);
size_t m3_wfst_search_state_size(const m3_wfst_search_desc* desc);
int m3_wfst_search_reset(const m3_wfst_search_desc* desc, void* state, size_t state_bytes, const void* graph, size_t graph_bytes,
                         const int32_t* slots, int n, m3_stream stream);
int m3_wfst_search_advance(const m3_wfst_search_desc* desc, void* state, size_t state_bytes, const void* graph, size_t graph_bytes,
                           const float* logp, int ld, int T_chunk, const int32_t* n_frames, m3_stream stream);
int m3_wfst_search_result(const m3_wfst_search_desc* desc, const void* state, size_t state_bytes, const void* graph,
                          size_t graph_bytes, int final, int max_words, int32_t* words, int32_t* frames, int32_t* n_words,
                          float* cost, int32_t* flags, int32_t* status, m3_stream stream);

/* m3_wfst_skip: CTC blank-frame skipping in front of the graph search (csrc/ctc_wfst_skip.hip; restated on the
 * host in tests/wfst_skip_ref.py).  The search above costs time in proportion to the frames it is given; a frame whose blank
 * posterior is near 1 moves no token anywhere but along blank arcs.  These calls choose, on the device, the rows of a chunk
 * that the search has to see, copy them to a dense buffer for m3_wfst_search_advance, and keep what is needed to go on in the
 * next chunk and to turn the search's word frames (numbers of DECODED frames) back into real frame numbers.  Skipping is an
 * approximation: the search's costs and, away from peaked posteriors, its words may differ from the unskipped search's.
 *
 * m3_wfst_skip_desc: B utterances, V columns, blank in [0, V), max_frames >= 0 entries of the frame map per utterance,
 *   log_blank_thresh = log of the blank posterior above which a frame is skipped (a float32; any value but NaN: +inf skips
 *   nothing).
 * state: caller-owned device memory, m3_wfst_skip_state_size bytes (0 = bad descriptor, or B = 0), 16-byte aligned.  Per
 *   utterance, at multiples of the per-utterance size (8 words + V + max_frames words, rounded up to 16 bytes):
 *     header, 8 int32 words: [0] last_blank  [1] last_best  [2] saved_frame  [3] n_seen  [4] n_kept  [5..7] 0
 *     saved row [V] float32: the last skipped row, valid while last_blank != 0
 *     map [max_frames] int32: map[j] = the real frame of the j-th row emitted since the reset
 *   reset: last_blank = 0, last_best = blank, saved_frame = n_seen = n_kept = 0 for all B utterances (slots NULL) or the n
 *   listed ones (device int32; an index outside [0, B) is skipped).  The saved row, the map and other utterances' bytes are
 *   not touched.
 * The rule.  The frames of an utterance in order, over all calls since its reset; row = the frame's log-probabilities,
 *   t = n_seen++ its number:
 *     row[blank] > log_blank_thresh (one float32 comparison in the log domain; false for a NaN): the frame is SKIPPED --
 *       last_blank = 1, and (row, t) is saved, replacing what was saved.
 *     otherwise best = the smallest index of the row's maximum, a NaN entry counting as -inf (0 when every entry does).
 *       If best != blank and last_blank != 0 and best == last_best, the saved row is emitted first, under its own frame
 *       number: two equal tokens that a blank separated stay two tokens.  Then row is emitted under t, last_best = best,
 *       last_blank = 0.
 *   emit (row, frame): the row's V values are copied, bit for bit, to the next row of out[b]; map[n_kept] = frame is stored
 *     only while n_kept < max_frames; n_kept++ counts on regardless.
 * select: logp [B][T_chunk][ld] float32 (ld >= V), n_frames[B] frames of each utterance that count, clamped to [0, T_chunk];
 *   out [B][T_chunk + 1][ld_out] float32 (ld_out >= V; a call emits at most n_frames + 1 rows, the + 1 being a row saved by
 *   an earlier call; rows behind the emitted ones and columns >= V are not written; out must not overlap logp);
 *   n_kept[B] = rows emitted by THIS call -- what m3_wfst_search_advance takes as n_frames with out as logp.  When the chunk
 *   ends with last_blank set by one of its own frames, that row is copied into the state.  One work-group of 1024 threads per
 *   utterance, one launch, no host sync, capturable.
 * map_frames: frames [B][ld_frames] int32 in place, n_words[B]: for i < min(n_words[b], ld_frames) a value r becomes map[r]
 *   when 0 <= r < min(n_kept, max_frames), else n_seen (with nothing seen that is 0, the frame the unskipped search gives a
 *   word made at reset; with frames seen but none kept it is the number of frames seen).  Other entries, and utterances
 *   with n_words < 0, are left alone.
 * counts: seen[B] = n_seen, kept[B] = n_kept (since the reset, over all calls).
 * Every call refuses, before any launch: a null descriptor, B outside [0, 32768], V outside [1, 2^24], blank outside [0, V),
 *   max_frames outside [0, 2^28], a NaN threshold, a state that is null, misaligned or too small, a null pointer, ld < V,
 *   ld_out < V, T_chunk < 0, ld_frames < 0, more slots than B. */
typedef struct m3_wfst_skip_desc {
  int32_t B, V, blank, max_frames;
  float log_blank_thresh;
} m3_wfst_skip_desc;
size_t m3_wfst_skip_state_size(const m3_wfst_skip_desc* desc);
int m3_wfst_skip_reset(const m3_wfst_skip_desc* desc, void* state, size_t state_bytes, const int32_t* slots, int n, m3_stream stream);
int m3_wfst_skip_select(const m3_wfst_skip_desc* desc, void* state, size_t state_bytes, const float* logp, int ld, int T_chunk,
                        const int32_t* n_frames, float* out, int ld_out, int32_t* n_kept, m3_stream stream);
int m3_wfst_skip_map_frames(const m3_wfst_skip_desc* desc, const void* state, size_t state_bytes, int32_t* frames, int ld_frames,
                            const int32_t* n_words, m3_stream stream);
int m3_wfst_skip_counts(const m3_wfst_skip_desc* desc, const void* state, size_t state_bytes, int32_t* seen, int32_t* kept,
                        m3_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* M3ASR_H_ */
