// Whole-encoder engine: the native runtime that stands where the TensorRT engine stood.
//
// Reference: builder.py:36-98 builds a TensorRT plan from model.encoder(network_helper, feat, feat_len)
// and infer.py:38-103 runs it with execute_v2.  The network being executed is
//   Net.forward            trainer_3m_fix/model/conformer_fmoe_localComm_catEmbed_domain_acc_hier.py:198-234
//   embed encoder          trainer_3m_fix/model/conformer_embed_domain_acc.py:149-181
//   FmoeConformerLayer     trainer_3m_fix/layer/fmoe_transformer.py:72-170
//   ConformerEncoderLayer  trainer_3m_fix/layer/transformer.py:179-275
// Here the same network is an ordered list of fused kernel stages over caller-owned buffers, captured
// once per (shape, buffers) into a hipGraph and replayed.  The residual stream x (S x D) is updated in
// place by GEMM / combine epilogues; LayerNorms ride in GEMM prologues except where their output is a
// tensor of its own (MoE input, block output).
#include <assert.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <variant>
#include <vector>

#include "../../include/m3asr.h"
#include "common.h"
#include "kernels.h"

namespace m3 {
struct MoeWorkspace {
  int32_t* mapping; int32_t* acc; int32_t* pos; float* slab; size_t bytes;
};
MoeWorkspace carve_moe_workspace(void* base, int S, int E, int D, int F);
}  // namespace m3

using namespace m3;

namespace {

struct Norm { const float* g = nullptr; const float* b = nullptr; };
// wf: the same weight in MFMA-fragment order (kernels.h GemmParams::w_frag), where the plan holds one: what the skinny fp32 form reads
struct Lin { const float* w = nullptr; const float* b = nullptr; const float* wsum = nullptr; const float* wbeta = nullptr; const float* wf = nullptr; };

struct BlockW {
  Norm n_ffm, n_mha, n_conv, n_ff, n_final, n_cnn;
  Lin mac1, mac2, qkv, pos, out, pw1, pw2, ff1, ff2;
  const float* pos_u = nullptr; const float* pos_v = nullptr;
  const float* dw_w = nullptr; const float* dw_b = nullptr;
  const float* left_fill = nullptr;   // causal conv module: GLU(pointwise_conv1.bias), what a zero-padded frame is at the depthwise conv's input
  Lin router;                       // w: [E_total][D + De]  (unfused route path)
  Lin router_x;                     // w: [E][D] x-half with norm_ff folded (+ wsum, bias)  (fused route path)
  const float *ew1 = nullptr, *eb1 = nullptr, *ew2 = nullptr, *eb2 = nullptr;
  const float *ew1f = nullptr, *ew2f = nullptr;   // fp32 experts in fragment order (both or neither): what expert_ffn_f32_kernel reads
  const float *es1 = nullptr, *es2 = nullptr;   // fp8 experts: per-row scales [E][F], [E][D]; mxfp4 experts: the e8m0 scale BYTES [E][F][D/32], [E][F/64][D][2]
  float h_scale = 0.f;                          // fp8 arithmetic: static scale of the hidden activations (0 = weight-only)
};

struct SubW { const float* c1w; const float* c1b; const float* c2w; const float* c2b; Lin out; int in_ch = 1; };

// One launch of a kernel family, as the family's host record (kernels.h).  A stage that is one such launch holds the record and
// nothing else: run_stage runs it from the record, and horizontal fusion (fuse_independent_pairs) pairs two stages by reading
// the same records -- a one-launch dense GEMM, the conv module's depthwise conv + LayerNorm + SiLU, the fp32 rel-pos attention
// core, and of the two subsamplers the first conv and the split-K GEMM + reduce stages (two launches before and after).
using Launch = std::variant<std::monostate, GemmLaunch, Conv1Args, DwArgs, AttArgs>;

struct Stage {
  std::string name;
  std::function<int(hipStream_t)> run;   // a stage that is NOT one family launch (MoE stages, layernorm, pack, taps, a fused pair)
  m3_stage_info info;   // kernel label + algorithmic bytes / FLOPs of the stage (m3_engine_stage_info)
  bool reads_embed = false;   // reads the embed encoder's output (pl.emb, or pl.eall computed from it): where the chains join
  Launch launch;              // the record of the one launch the stage is (empty: the stage is what `run` does)
  bool pairable = false;      // a record stage that may share its launch with a stage of the other encoder
  bool router_prefix = false;   // the "router_e_prefix" stage (Bound::prefix_stage)
  // a router stage that starts from the accumulator prefix of "router_e_prefix": recomputes its layer's slice (m3_engine_run)
  std::function<int(hipStream_t)> refresh_prefix;
};
const GemmLaunch& gemm_of(const Stage& st) { return std::get<GemmLaunch>(st.launch); }
bool is_splitk(const Stage& st) { return std::holds_alternative<GemmLaunch>(st.launch) && gemm_of(st).plan.kernel == GemmKernel::SplitKF32; }

m3_stage_info stage_info(const char* kernel, int launches, double bytes, double flops, bool per_row = true) {
  m3_stage_info i;
  i.kernel = kernel; i.launches = launches; i.per_row = per_row ? 1 : 0; i.alg_bytes = bytes; i.flops = flops;
  return i;
}

struct Buf { void* ptr; size_t bytes; };

// What identifies a binding: the shape, the caller's buffers and the mode.  Two forwards with equal keys run the same stage
// list; everything else in a binding is derived from its key (and the engine's weights and config).
struct BindKey {
  int B = 0, T = 0;
  const float* feat = nullptr; const int32_t* feat_len = nullptr; float* logits = nullptr;
  void* ws = nullptr; size_t ws_bytes = 0;
  int ep_cap = 0;        // expert parallel: rows per wire chunk (m3_engine_set_ep_capacity at the time of binding)
  // chunk-by-chunk (streaming) binding: T = 4 c + 3 input frames -> the c frames of one chunk; attention reads / extends the
  // K / V history and the causal depthwise conv its K-1 frame cache, both in the caller-owned state (m3_engine_forward_chunk)
  void* sstate = nullptr; int s_hist = 0, s_maxf = 0;
  bool s_slots = false;   // slot mode (m3_engine_forward_chunk_slots): every utterance slot of the state has its own chunk counter
  bool operator==(const BindKey& o) const {
    return B == o.B && T == o.T && feat == o.feat && feat_len == o.feat_len && logits == o.logits && ws == o.ws &&
           ws_bytes == o.ws_bytes && ep_cap == o.ep_cap && sstate == o.sstate && s_hist == o.s_hist && s_maxf == o.s_maxf &&
           s_slots == o.s_slots;
  }
};

}  // namespace

struct m3_engine {
  m3_engine_config cfg;
  std::unordered_map<std::string, m3_weight_entry> table;
  std::vector<std::string> names;  // keeps c_str storage alive
  SubW sub_e, sub_m;
  std::vector<BlockW> eblocks, mblocks;
  Norm e_after, m_after;
  Lin out_linear;
  const float* pe = nullptr;
  int64_t pe_rows = 0;
  const float* pos_all = nullptr;   // [(embed_blocks + num_blocks) * D][D]: every block's linear_pos weight
  const float* cmvn_mean = nullptr; const float* cmvn_istd = nullptr;   // optional global CMVN (fused into conv1)
  const float* output_bias = nullptr;                                     // optional [V] added to the output (-log prior)
  const float* router_e_all = nullptr;   // [num_blocks * E][De]: embed half of every layer's router (fused route path)

  // state of the bound shape (buffers + stage list + captured graph); up to cfg.shape_cache more are parked, so a server
  // that alternates between a few (B, T) buckets with static I/O buffers replays graphs instead of re-capturing them
  struct Bound {
    BindKey key;
    int Tp = 0, S = 0;   // subsampled frames per utterance, rows of the residual stream (B * T')
    bool a16 = false;   // activations that only feed GEMMs are kept as bf16 (h1, ctx, dw, c1, c2) + a bf16 copy of x
    bool dma = false;   // a16 and the block GEMMs run on the LDS-DMA kernel: every kernel that writes xb also leaves its row statistics
    bool packed = false;   // ragged batch: the blocks run on the packed valid rows (cfg.packed_rows)
    bool xn_skipped = false;   // the router kernel was told not to write the fp32 MoE input rows (M3_ROUTER_SKIP_XN=1)
    // fork_embed: stages [fork_first, fork_mid) = the embed encoder (side branch of the captured graph), [fork_mid, join_at) =
    // what the main encoder does before it needs the embedding (embed_join); -1 = one linear chain
    int fork_first = -1, fork_mid = -1, join_at = -1;
    int prefix_stage = -1;   // index of "router_e_prefix" (-1: the routers run their whole K)
    // fold_pos_proj: linear_pos(pe[:T']) of every block, computed once per T'.  ENGINE-owned device memory (shared by all
    // bindings of the same T', freed with the last of them): a caller that reuses one workspace for several shapes, as a
    // TensorRT execution context does, must not be able to overwrite it between two forwards of a revived binding
    std::shared_ptr<float> pfold;
    std::vector<Stage> stages;
    std::unordered_map<std::string, Buf> buffers;
    int n_kernels = 0;
    hipGraphExec_t graph_exec = nullptr;
    bool graph_valid = false;
    uint64_t last_use = 0;
    bool matches(const BindKey& k) const { return !stages.empty() && key == k; }
  };
  Bound cur;
  std::vector<Bound> parked;
  uint64_t use_clock = 0;
  int n_captures = 0;                                      // graphs captured so far (observability / tests)
  int ep_capacity = 0;                                     // rows per wire chunk agreed by the ranks for the NEXT bindings (0 = own rows)
  hipStream_t side = nullptr;                              // second capture stream: the embed branch of forked graphs
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  std::unordered_map<int, std::weak_ptr<float>> pfold_by_tp;   // T' -> folded positional projection still in use
};

namespace {

// The engine's run-time switches: environment variables read once per process, when the first stage list is built.
struct Switches {
  // M3_GATE_INDEX_MAX_ROWS (512): rows up to which SoftmaxTopK + ScatterMapping run as ONE single-work-group launch (beyond:
  // row-parallel top-1 + index kernel).  A/B at configs[2] (1984 padded rows): 2048 -> 315 instead of 333 launches but 3.856 vs
  // 3.794 ms per forward (one work-group walks 1984 x 32 logits): the default stays 512.
  int gate_index_max_rows;
  // M3_SELF_ROUTE (1): 0 puts the single-work-group SoftmaxTopK + ScatterMapping launch back in front of the short-input fp32
  // expert launch, which otherwise routes for itself (staged and split route)
  bool self_route;
  // M3_HFUSE (1): 0 = no horizontal fusion of the embed encoder with the main encoder's prefix (fuse_independent_pairs)
  bool hfuse;
  // M3_ROUTER_MIN_ROWS (2048): the dedicated router kernel from this many rows on.  A/B at the three BASELINE shapes, one
  // device: configs[4]-share 46.0 -> 29.1 us per layer, forward 8.83 -> 8.52 ms; configs[2] 14.1 vs 14.9 us and B = 1 +1.5 us
  // per layer: there the 16-column work-groups of gemm.hip spread the 128-KB weight pull over more CUs.
  int router_min_rows;
  // M3_ROUTER_XQ (1): fp8 arithmetic, all experts local, the fused expert kernel next: the router kernel also leaves the rows
  // quantised (e4m3 + a scale per row), the expert kernel reads 512 B per row instead of 2 KB.  0: as before
  bool router_xq;
  // M3_ROUTER_SKIP_XN (0): 1 = ... and the router kernel no longer writes the fp32 rows (the "xn" buffer, which the
  // calibration tools read, is then not offered)
  bool router_skip_xn;
  // M3_FUSED8_ADAPT (0): 1 = all experts local, fused fp8 kernel: the kernel may split F finer than the host's choice when the
  // routing leaves CUs without an item (the expert-parallel receive side always keeps the host's split: its result stays
  // comparable bit for bit with any other grouping of the same rows under the same split).  A latency / throughput trade, OFF
  // by default: measured at configs[4]'s share on one box, the launch 38.5 -> 27.8 us and one forward alone 6.70 -> 6.57 ms,
  // but 4.58 -> 4.45 M frames/s at four contexts (twice the partial-output slabs; the idle CUs were being used by the other
  // contexts' kernels)
  bool fused8_adapt;
  // M3_GLU_DEFER (1): 0 = the conv module's pointwise_conv1 keeps its GLU epilogue at every shape.  1: fp32 plans, symmetric
  // conv module, 16-row-tile skinny GEMM, 256 <= D <= 1024: pointwise_conv1 runs as the plain folded-LayerNorm form and the
  // depthwise kernel applies the GLU to the taps it loads (glu_deferred)
  bool glu_defer;
  // M3_FRONT_PAIR (1): 0 = the two subsamplers keep their five launches each.  1: where both second convs plan as split-K
  // (C >= 512) and the embed chain is interleaved with the main prefix (M3_HFUSE), conv1, conv2 + reduce and Linear + reduce of
  // the two run as one launch each
  bool front_pair;
  // M3_ROUTER_PREFIX (1): 0 = every staged fp32 router GEMM walks its whole K.  1 (fp32, S <= 128 rows, De = D >= 256, the router
  // planning as the one-group 16-row form): the embed half of all layers' router products is run once per forward by
  // "router_e_prefix", as the accumulator registers the router GEMMs then start from (GemmParams::acc_init)
  bool router_prefix;
  // M3_GLU_SIG_EPI (1): 0 = a deferred GLU's gate columns leave pointwise_conv1 raw and the depthwise kernel sigmoids them per
  // tap.  1: pointwise_conv1's epilogue stores sigmoid(gate) (GemmParams::sig_col0), the depthwise kernel multiplies
  bool glu_sig_epi;
  // M3_W_FRAG (1): 0 = the fragment-ordered copies of the fp32 weights (names ending in "_frag") are ignored: the skinny GEMMs and
  // the one-launch expert kernel read the row-major / slice-major tensors, as every other form always does
  bool w_frag;
};
const Switches& switches() {
  static const Switches sw = [] {
    auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    Switches w;
    w.gate_index_max_rows = num("M3_GATE_INDEX_MAX_ROWS", 512);
    w.self_route = num("M3_SELF_ROUTE", 1) != 0;
    w.hfuse = num("M3_HFUSE", 1) != 0;
    w.router_min_rows = num("M3_ROUTER_MIN_ROWS", 2048);
    w.router_xq = num("M3_ROUTER_XQ", 1) != 0;
    w.router_skip_xn = num("M3_ROUTER_SKIP_XN", 0) != 0;
    w.fused8_adapt = num("M3_FUSED8_ADAPT", 0) != 0;
    w.glu_defer = num("M3_GLU_DEFER", 1) != 0;
    w.front_pair = num("M3_FRONT_PAIR", 1) != 0;
    w.router_prefix = num("M3_ROUTER_PREFIX", 1) != 0;
    w.glu_sig_epi = num("M3_GLU_SIG_EPI", 1) != 0;
    w.w_frag = num("M3_W_FRAG", 1) != 0;
    return w;
  }();
  return sw;
}

// dtype: what the engine will read the tensor as (GEMM weights follow cfg.weight_dtype, everything else is fp32)
bool lookup(const m3_engine* e, const std::string& name, int64_t numel, const float** out, int dtype = M3_F32) {
  auto it = e->table.find(name);
  if (it == e->table.end()) {
    set_error("engine: weight '%s' missing from the plan", name.c_str());
    return false;
  }
  if (numel >= 0 && it->second.numel != numel) {
    set_error("engine: weight '%s' has %lld elements, expected %lld", name.c_str(), (long long)it->second.numel,
              (long long)numel);
    return false;
  }
  if (it->second.dtype != dtype) {
    set_error("engine: weight '%s' has dtype %d, the engine (weight_dtype=%d) expects %d", name.c_str(),
              (int)it->second.dtype, (int)e->cfg.weight_dtype, dtype);
    return false;
  }
  *out = (const float*)it->second.data;
  return true;
}

#define GET(dst, name, numel) \
  do { if (!lookup(e, (name), (numel), &(dst))) return false; } while (0)
// dense GEMM weights: fp32, or bf16 in the 16-bit, fp8 and mxfp4 modes; expert weights follow weight_dtype itself
#define GETW(dst, name, numel) \
  do { if (!lookup(e, (name), (numel), &(dst), e->cfg.weight_dtype == M3_F32 ? M3_F32 : M3_BF16)) return false; } while (0)
#define GETE(dst, name, numel) \
  do { if (!lookup(e, (name), (numel), &(dst), e->cfg.weight_dtype)) return false; } while (0)

bool load_norm(const m3_engine* e, const std::string& p, int d, Norm* n) {
  GET(n->g, p + "weight", d);
  GET(n->b, p + "bias", d);
  return true;
}
// the optional fragment-ordered copy of an fp32 tensor (Engine.__init__ derives it; absent: the stages read `name` itself)
const float* lookup_frag(const m3_engine* e, const std::string& name, int64_t numel) {
  if (!switches().w_frag || e->cfg.weight_dtype != M3_F32) return nullptr;
  auto it = e->table.find(name + "_frag");
  return it != e->table.end() && it->second.numel == numel && it->second.dtype == M3_F32 ? (const float*)it->second.data : nullptr;
}
bool load_lin(const m3_engine* e, const std::string& p, int64_t n_out, int64_t n_in, bool bias, Lin* l) {
  GETW(l->w, p + "weight", n_out * n_in);
  l->wf = lookup_frag(e, p + "weight", n_out * n_in);
  if (bias) GET(l->b, p + "bias", n_out);
  return true;
}
// Linear with a LayerNorm folded in (plan.py fold_layernorm): weight = W*gamma, bias = b + W.beta, wsum = rowsum(W*gamma)
bool load_lin_ln(const m3_engine* e, const std::string& p, int64_t n_out, int64_t n_in, bool wbeta, Lin* l,
                 bool fp32_only = false) {
  if (fp32_only) {
    GET(l->w, p + "ln.weight", n_out * n_in);
  } else {
    GETW(l->w, p + "ln.weight", n_out * n_in);
  }
  if (!fp32_only) l->wf = lookup_frag(e, p + "ln.weight", n_out * n_in);
  GET(l->b, p + "ln.bias", n_out);
  GET(l->wsum, p + "ln.wsum", n_out);
  if (wbeta) GET(l->wbeta, p + "ln.wbeta", n_out);
  return true;
}

bool load_block(const m3_engine* e, const std::string& p, int D, int F, int K, bool cnn_ln, bool moe, int De, BlockW* b, bool causal) {
  const m3_engine_config& c = e->cfg;
  // norm_ff_macaron / norm_mha / norm_conv (and norm_ff of dense blocks) have no tensor of their own: folded into weights
  if (!load_norm(e, p + "norm_final.", D, &b->n_final)) return false;
  if (moe && !load_norm(e, p + "norm_ff.", D, &b->n_ff)) return false;
  if (!load_lin_ln(e, p + "feed_forward_macaron.w_1.", F, D, false, &b->mac1) ||
      !load_lin(e, p + "feed_forward_macaron.w_2.", D, F, true, &b->mac2) ||
      !load_lin_ln(e, p + "self_attn.qkv.", 3 * D, D, false, &b->qkv) ||
      !load_lin(e, p + "self_attn.linear_out.", D, D, true, &b->out) ||
      !load_lin_ln(e, p + "conv_module.pointwise_conv1.", 2 * D, D, true, &b->pw1) ||
      !load_lin(e, p + "conv_module.pointwise_conv2.", D, D, true, &b->pw2))
    return false;
  GET(b->pos_u, p + "self_attn.pos_bias_u", D);
  GET(b->pos_v, p + "self_attn.pos_bias_v", D);
  GET(b->dw_w, p + "conv_module.depthwise_conv.weight_kc", (int64_t)K * D);
  GET(b->dw_b, p + "conv_module.depthwise_conv.bias", D);
  if (cnn_ln && !load_norm(e, p + "conv_module.norm.", D, &b->n_cnn)) return false;
  if (causal) GET(b->left_fill, p + "conv_module.left_fill", D);
  if (!moe) {
    if (!load_lin_ln(e, p + "feed_forward.w_1.", F, D, false, &b->ff1) ||
        !load_lin(e, p + "feed_forward.w_2.", D, F, true, &b->ff2))
      return false;
  } else {
    const int world = c.ep_world_size > 0 ? c.ep_world_size : 1;
    const int64_t Etot = (int64_t)c.num_experts * world;
    GET(b->router.w, p + "feed_forward.router_weights_t", Etot * (D + De));
    if (c.router_with_bias) GET(b->router.b, p + "feed_forward.router_bias", Etot);
    if (c.fuse_route && !load_lin_ln(e, p + "feed_forward.router_x.", Etot, D, false, &b->router_x, true)) return false;
    const int64_t E = c.num_experts;
    // (mxfp4: two codes per byte, one scale byte per 32 k -- the tensors are bytes)
    const int64_t ew_numel = c.weight_dtype == M3_MXFP4 ? E * F * D / 2 : E * F * D;
    GETE(b->ew1, p + "feed_forward.experts.w_1.weight", ew_numel);
    if (c.weight_dtype == M3_MXFP4) {
      GETE(b->es1, p + "feed_forward.experts.w_1.scale", E * F * D / 32);
      GETE(b->es2, p + "feed_forward.experts.w_2.scale", E * F * D / 32);
    }
    if (c.weight_dtype == M3_FP8) {
      GET(b->es1, p + "feed_forward.experts.w_1.scale", E * F);
      GET(b->es2, p + "feed_forward.experts.w_2.scale", E * D);
      if (c.fp8_activations) {          // the calibrated scale of H: one fp32 number per layer, read once at set-up
        const float* hs = nullptr;
        GET(hs, p + "feed_forward.experts.h_scale", 1);
        if (hipMemcpy(&b->h_scale, hs, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess || !(b->h_scale > 0.f)) {
          set_error("engine: '%sfeed_forward.experts.h_scale' must hold one positive number", p.c_str());
          return false;
        }
      }
    }
    GET(b->eb1, p + "feed_forward.experts.w_1.bias", E * F);
    GETE(b->ew2, p + "feed_forward.experts.w_2.weight_sliced", ew_numel);
    GET(b->eb2, p + "feed_forward.experts.w_2.bias", E * D);
    b->ew1f = lookup_frag(e, p + "feed_forward.experts.w_1.weight", ew_numel);
    b->ew2f = lookup_frag(e, p + "feed_forward.experts.w_2.weight", ew_numel);
    if (!b->ew1f || !b->ew2f) b->ew1f = b->ew2f = nullptr;
  }
  return true;
}

// bins per input channel of a subsampler's first conv, and what the two stride-2 3x3 convs leave of them
inline int sub_fc(int idim, int in_ch) { return idim / in_ch; }
inline int sub_f1(int fc) { return (fc - 3) / 2 + 1; }
inline int sub_f2(int fc) { return (sub_f1(fc) - 3) / 2 + 1; }

// The first conv's input channels are read off its weight: conv.0.weight_9c holds 9 * in_ch * D numbers (m3_engine_config does
// not change for them).  The idim columns of a frame are then in_ch blocks of Fc = idim / in_ch bins.
bool load_sub(const m3_engine* e, const std::string& p, int D, int idim, SubW* s) {
  auto it = e->table.find(p + "conv.0.weight_9c");
  const int64_t numel = it == e->table.end() ? 9 * (int64_t)D : it->second.numel;
  s->in_ch = (int)(numel / (9 * (int64_t)D));
  if (numel % (9 * (int64_t)D) || s->in_ch < 1 || s->in_ch > 3) {
    set_error("engine: '%sconv.0.weight_9c' has %lld elements: 9 * in_ch * %d with 1 to 3 input channels expected", p.c_str(), (long long)numel, D);
    return false;
  }
  if (idim % s->in_ch || sub_fc(idim, s->in_ch) < 7) {
    set_error("engine: '%sconv.0.weight_9c' has %d input channels: input_dim=%d must be a multiple of it with at least 7 bins per channel",
              p.c_str(), s->in_ch, idim);
    return false;
  }
  const int F2 = sub_f2(sub_fc(idim, s->in_ch));
  GET(s->c1w, p + "conv.0.weight_9c", 9 * (int64_t)s->in_ch * D);
  GET(s->c1b, p + "conv.0.bias", D);
  GETW(s->c2w, p + "conv.2.weight_ohwi", 9 * (int64_t)D * D);
  GET(s->c2b, p + "conv.2.bias", D);
  return load_lin(e, p + "out.0.", D, (int64_t)D * F2, true, &s->out);
}
#undef GET
#undef GETW
#undef GETE

inline int sub_len(int t) { return ((t - 3) / 2 + 1 - 3) / 2 + 1; }

struct Carver {
  char* base; size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <typename T> T* take(size_t n) {
    T* p = (T*)(base ? base + off : nullptr);
    off += align_up(n * sizeof(T), 256);
    return p;
  }
};

// Buffer plan of one bound shape (identical code computes the size and the addresses).
struct Plan {
  int32_t* lens;
  float *c1, *c2, *x, *emb, *h1, *qkv, *pbuf, *ctx, *glu, *dw, *xn, *rl, *eall;
  // the routers' accumulator prefix [num_blocks][rprefix_layer floats] (null: not taken), router_prefix_layer_floats
  float* rprefix; size_t rprefix_layer;
  void* xb;                             // bf16 copy of the residual stream (16-bit modes, long batches)
  int32_t* moe_fs;                      // fp8 plans: the F split the fused expert kernel chose on the device (slab count for the combine)
  unsigned char* xq; float* xq_scale;   // fp8 plans: the MoE input rows as e4m3 [S][D] + per-row scales (router kernel -> fused fp8 expert kernel)
  float* xstats;                        // [S][kXbStatParts][2]: row statistics of xb for the folded-LayerNorm GEMMs (gemm_bf16_dma.hip)
  int32_t* gate_idx; float* gate_val;   // [n_moe][S]
  void* moe_ws; size_t moe_ws_bytes;
  float* splitk; size_t splitk_bytes;   // split-K partials of conv2 / subsampling Linear (fp32 plans, short inputs)
  float* taps;                          // [n_blocks_total][S][D] when debug_taps
  float* pfold;                         // [n_blocks_total][Tp][D] when fold_pos_proj
  // packed ragged batches: row plan, padded staging of the subsamplers' output, packed logits
  int32_t *row0, *pad_of; float* xpad; void* xbpad; float* lpk;
  // expert parallel (ep_world_size > 1): send-side index over GLOBAL expert ids, the two wire buffers [world][1 + C][D]
  // and the receive-side gate; the MoE workspace is then sized for the world * (1 + C) rows a rank can receive
  int32_t *ep_acc, *ep_mapping, *ep_pos, *ep_map_send, *ep_gate_recv, *ep_overflow; float *wire_a, *wire_b; int ep_cap, ep_rows;
  // fork_embed: the embed encoder runs on its own graph branch beside the main subsampler and block 0 up to its router
  // (conformer_fmoe_..._hier.py:206-215: embed is needed first by blocks.0's router), so it owns a second set of scratch
  bool fork;
  bool hfuse;                           // embed chain and main prefix interleaved in one stream (separate scratch, as with fork)
  float *e_c1, *e_c2, *e_x, *e_h1, *e_qkv, *e_ctx, *e_glu, *e_dw, *e_xpad, *e_splitk, *e_xstats; void *e_xb, *e_xbpad;
  size_t bytes;
};

// Only on request.  Measured at configs[1] (profiles/r03_ab_headline.txt): one forward alone 2.39 -> 2.33 ms (the ~13 launches
// of the main encoder's start overlap the embed encoder), but four execution contexts x two branches are eight concurrently
// active queues, past the four the part runs truly concurrently: 207 k -> 69 k frames/s.
bool use_fork_embed(const m3_engine_config& c, int B, int S) { return c.fork_embed > 0 && !c.debug_taps; }
// the blocks run on packed rows: B > 1 (or forced), no per-block taps (they are read as (B, T', D)), staged route
bool use_packed_rows(const m3_engine_config& c, int B) {
  if (c.packed_rows < 0 || (c.packed_rows == 0 && B <= 1)) return false;
  return !c.debug_taps && c.fuse_route == 0 && B <= 1024;   // (expert-parallel ranks too: rows past the live count never travel)
}

// horizontal fusion of the embed encoder with the main encoder's independent prefix (fuse_independent_gemm_pairs): fp32 plans
// whose block GEMMs are 16-row-tile launches (S <= 128 rows).  Needs the embed chain's scratch apart from the main chain's.
bool use_hfuse(const m3_engine_config& c, int B, int S) {
  return switches().hfuse && !c.debug_taps && c.weight_dtype == M3_F32 && c.embed_blocks > 0 && c.num_blocks > 0 && S <= 128 && c.fork_embed <= 0 &&
         !use_packed_rows(c, B);
}

size_t router_prefix_layer_floats(const m3_engine_config& c, int S, const Plan& pl);

Plan make_plan(const m3_engine& eng, void* base, int B, int T, int ep_capacity = 0) {
  const m3_engine_config& c = eng.cfg;
  Plan p;
  Carver cv(base);
  const int Tp = sub_len(T), S = B * Tp;
  // the subsamplers' buffers hold either encoder's: sized by the one with fewer input channels (more bins per channel)
  const int fc_m = sub_fc(c.input_dim, eng.sub_m.in_ch), fc_e = sub_fc(c.input_dim, eng.sub_e.in_ch), fc = fc_m > fc_e ? fc_m : fc_e;
  const int T1 = (T - 3) / 2 + 1, F1 = sub_f1(fc), F2 = sub_f2(fc);
  const int D = c.attention_dim > c.embed_dim ? c.attention_dim : c.embed_dim;
  const int F = c.hidden_units > c.embed_linear_units ? c.hidden_units : c.embed_linear_units;
  const int world = c.ep_world_size > 0 ? c.ep_world_size : 1;
  const int Etot = c.num_experts * world;
  p.lens = cv.take<int32_t>(B);
  p.c1 = cv.take<float>((size_t)B * T1 * F1 * D);
  p.c2 = cv.take<float>((size_t)S * F2 * D);
  p.x = cv.take<float>((size_t)S * D);
  p.emb = cv.take<float>((size_t)S * D);
  p.xb = cv.take<uint16_t>((size_t)S * D);
  p.xstats = cv.take<float>((size_t)S * 2 * kXbStatParts);
  p.h1 = cv.take<float>((size_t)S * F);
  p.qkv = cv.take<float>((size_t)S * 3 * D);
  p.pbuf = cv.take<float>((size_t)Tp * D * (c.num_blocks + c.embed_blocks));
  p.ctx = cv.take<float>((size_t)S * D);
  // (pointwise_conv1's raw value | gate columns where the GLU is deferred to the depthwise kernel: glu_deferred)
  const size_t glu_floats = (size_t)S * D * (switches().glu_defer && c.weight_dtype == M3_F32 && D >= 256 ? 2 : 1);
  p.glu = cv.take<float>(glu_floats);
  p.dw = cv.take<float>((size_t)S * D);
  p.xn = cv.take<float>((size_t)S * D);
  p.xq = nullptr; p.xq_scale = nullptr; p.moe_fs = nullptr;
  if (c.weight_dtype == M3_FP8) p.moe_fs = cv.take<int32_t>(64);
  if (c.weight_dtype == M3_FP8 && D == 512) {
    p.xq = cv.take<unsigned char>((size_t)S * D);
    p.xq_scale = cv.take<float>((size_t)S);
  }
  p.rl = cv.take<float>((size_t)S * Etot);
  p.eall = cv.take<float>((size_t)S * Etot * c.num_blocks);
  p.gate_idx = cv.take<int32_t>((size_t)c.num_blocks * S);
  p.gate_val = cv.take<float>((size_t)c.num_blocks * S);
  // rows per wire chunk: what the ranks agreed on (m3_engine_set_ep_capacity).  0 = this rank's own row count (no row can
  // be dropped); a smaller agreed capacity is a BOUNDED wire: a chunk that needs more rows reports it in "ep.overflow" and the
  // driver repeats the forward with a larger one (m3asr/ep.py)
  const bool ep = world > 1 || c.ep_stages > 0;
  p.ep_cap = ep ? (ep_capacity > 0 ? ep_capacity : S) : 0;
  p.ep_rows = ep ? world * (p.ep_cap + 1) : 0;
  p.moe_ws_bytes = carve_moe_workspace(nullptr, ep ? p.ep_rows : S, c.num_experts, c.attention_dim, c.hidden_units).bytes;
  p.moe_ws = cv.take<char>(p.moe_ws_bytes * (size_t)(c.debug_taps ? c.num_blocks : 1));
  p.ep_acc = p.ep_mapping = p.ep_pos = p.ep_map_send = p.ep_gate_recv = p.ep_overflow = nullptr; p.wire_a = p.wire_b = nullptr;
  if (ep) {
    p.ep_overflow = cv.take<int32_t>(64);
    p.ep_acc = cv.take<int32_t>((size_t)Etot + 1);
    p.ep_mapping = cv.take<int32_t>(S);
    p.ep_pos = cv.take<int32_t>(S);
    p.ep_map_send = cv.take<int32_t>(S);
    p.ep_gate_recv = cv.take<int32_t>(p.ep_rows);
    p.wire_a = cv.take<float>((size_t)p.ep_rows * c.attention_dim);
    p.wire_b = cv.take<float>((size_t)p.ep_rows * c.attention_dim);
  }
  {
    size_t n1 = 0, n2 = 0;
    if (c.weight_dtype == M3_F32) {
      for (const int f2 : {sub_f2(fc_m), sub_f2(fc_e)}) {   // (one problem twice unless the encoders differ in in_ch)
        GemmParams g;   // conv2 as implicit GEMM
        g.mode = GEMM_A_CONV3X3S2; g.lda = 4; g.conv_C = D; g.M = S * f2; g.N = D; g.K = 9 * D; g.ldy = D;
        n1 = std::max(n1, plan_gemm(g, SIZE_MAX).ws_bytes);
        GemmParams l;   // Linear(C*F2 -> D)
        l.lda = f2 * D; l.M = S; l.N = D; l.K = f2 * D; l.ldy = D;
        n2 = std::max(n2, plan_gemm(l, SIZE_MAX).ws_bytes);
      }
    }
    p.splitk_bytes = n1 > n2 ? n1 : n2;
    p.splitk = p.splitk_bytes ? cv.take<float>(p.splitk_bytes / sizeof(float)) : nullptr;
  }
  p.taps = c.debug_taps ? cv.take<float>((size_t)(c.num_blocks + c.embed_blocks) * S * D) : nullptr;
  p.pfold = nullptr;
  p.row0 = p.pad_of = nullptr; p.xpad = p.lpk = nullptr; p.xbpad = nullptr;
  if (use_packed_rows(c, B)) {
    p.row0 = cv.take<int32_t>(B + 1);
    p.pad_of = cv.take<int32_t>(S);
    p.xpad = cv.take<float>((size_t)S * D);
    p.xbpad = cv.take<uint16_t>((size_t)S * D);
    p.lpk = cv.take<float>((size_t)S * c.output_dim);
  }
  p.fork = use_fork_embed(c, B, S);
  p.hfuse = !p.fork && use_hfuse(c, B, S);
  p.e_c1 = p.c1; p.e_c2 = p.c2; p.e_x = p.x; p.e_h1 = p.h1; p.e_qkv = p.qkv; p.e_ctx = p.ctx; p.e_glu = p.glu; p.e_dw = p.dw;
  p.e_xb = p.xb; p.e_xpad = p.xpad; p.e_xbpad = p.xbpad; p.e_splitk = p.splitk; p.e_xstats = p.xstats;
  if (p.fork || p.hfuse) {
    p.e_c1 = cv.take<float>((size_t)B * T1 * F1 * D);
    p.e_c2 = cv.take<float>((size_t)S * F2 * D);
    p.e_x = cv.take<float>((size_t)S * D);
    p.e_xb = cv.take<uint16_t>((size_t)S * D);
    p.e_xstats = cv.take<float>((size_t)S * 2 * kXbStatParts);
    p.e_h1 = cv.take<float>((size_t)S * F);
    p.e_qkv = cv.take<float>((size_t)S * 3 * D);
    p.e_ctx = cv.take<float>((size_t)S * D);
    p.e_glu = cv.take<float>(glu_floats);
    p.e_dw = cv.take<float>((size_t)S * D);
    if (p.splitk_bytes) p.e_splitk = cv.take<float>(p.splitk_bytes / sizeof(float));
    if (use_packed_rows(c, B)) {      // (not `if (p.xpad)`: the sizing pass carves from a null base)
      p.e_xpad = cv.take<float>((size_t)S * D);
      p.e_xbpad = cv.take<uint16_t>((size_t)S * D);
    }
  }
  p.rprefix_layer = router_prefix_layer_floats(c, S, p);
  p.rprefix = p.rprefix_layer ? cv.take<float>(p.rprefix_layer * (size_t)c.num_blocks) : nullptr;
  p.bytes = cv.off;
  return p;
}

// Layout of the caller-owned streaming state (identical code computes the size and the addresses): the device-side chunk
// counter, then per block (embed blocks first) the K | V history [B][hist][2 D] and the depthwise conv's ping-pong cache
// [2][B][K-1][D] (post-GLU frames; the reference caches the module's INPUT and re-runs pointwise_conv1 + GLU on it,
// convolution.py:118-123 -- the same numbers, since both are per-frame operations).  Behind them, so that every offset above
// is what it was before slot mode existed, three words per utterance slot: chunks decoded, status (1 = asked to run past
// max_frames), output frames decoded.  Lockstep calls never touch them except m3_engine_stream_reset, which zeroes them.
struct StreamState {
  int32_t* step = nullptr;
  std::vector<float*> kv, conv;
  int32_t *slot_pos = nullptr, *slot_status = nullptr, *slot_frames = nullptr;   // [B] each, one allocation of 3 B words
  size_t bytes = 0;
};
StreamState carve_stream_state(const m3_engine_config& c, void* base, int B, int hist) {
  Carver cv(base);
  StreamState st;
  st.step = cv.take<int32_t>(64);
  const int nb = c.embed_blocks + c.num_blocks, D = c.attention_dim, K = c.cnn_module_kernel;
  for (int i = 0; i < nb; ++i) st.kv.push_back(cv.take<float>((size_t)B * hist * 2 * D));
  for (int i = 0; i < nb; ++i) st.conv.push_back(cv.take<float>((size_t)2 * B * (K - 1) * D));
  st.slot_pos = cv.take<int32_t>((size_t)3 * B);
  st.slot_status = st.slot_pos ? st.slot_pos + B : nullptr;
  st.slot_frames = st.slot_pos ? st.slot_pos + 2 * B : nullptr;
  st.bytes = cv.off;
  return st;
}

// the same plan with the embed branch's scratch under the usual names (what the embed encoder's stages are built from)
Plan embed_view(const Plan& pl) {
  Plan q = pl;
  q.c1 = pl.e_c1; q.c2 = pl.e_c2; q.x = pl.e_x; q.h1 = pl.e_h1; q.qkv = pl.e_qkv; q.ctx = pl.e_ctx; q.glu = pl.e_glu; q.dw = pl.e_dw;
  q.xb = pl.e_xb; q.xpad = pl.e_xpad; q.xbpad = pl.e_xbpad; q.splitk = pl.e_splitk; q.xstats = pl.e_xstats;
  return q;
}

// How one MoE layer routes its rows (positionwise_feed_forward.py:209-265: router, SoftmaxTopK, ScatterMapping), decided once
// per layer by choose_moe_route; the stage builders of build_block follow it.
enum class RouterForm {
  Gemm,     // staged: router GEMM on cat([embed, x]) with norm_ff as its prologue, which also writes xn
  Kernel,   // the dedicated router kernel: one work-group per 16 rows and all experts, every activation byte read once (moe_router.hip)
  Fused,    // fuse_route = 1: router (x half, norm_ff folded) + SoftmaxTopK + ScatterMapping in ONE launch ("moe_route")
  Split,    // fuse_route = 2: a K = D GEMM on x with norm_ff folded, the embed half added as its epilogue residual
};
enum class GateForm {   // where SoftmaxTopK (top-1) + ScatterMapping (index) happen
  RouterTail,   // top-1 in the router kernel's tail, then the index launch
  GateIndex,    // both in one single-work-group launch ("moe_gate_index")
  Top1Index,    // row-parallel top-1 launch, then the index launch
  InExpert,     // inside the expert launch: every work-group derives its expert's rows from the router logits
  InRoute,      // inside "moe_route"
};
struct MoeRoute {
  RouterForm router = RouterForm::Gemm;
  GateForm gate = GateForm::Top1Index;
  bool ep = false;            // expert parallel ("moe_ep.*": rows cross the wire) instead of all experts local ("moe_local.*")
  bool router_top1 = false;   // the router kernel writes gate_idx / gate_value in its tail (gate == RouterTail; with forced
                              // switches also in front of a self-routing expert launch)
  bool use_xq = false;        // the router kernel also leaves the rows quantised for the fused fp8 expert kernel
  bool skip_xn = false;       // ... and does not write the fp32 rows xn
  bool fs_dev = false;        // the fused fp8 kernel chooses its F split on the device (the combine reads the slab count)
  bool needs_e_all = false;   // the embed half of the router product comes from the once-per-forward "router_e_all" GEMM
  // fused / split route: no xn; the expert kernel reads the raw residual stream and applies norm_ff while it gathers rows
  bool norm_in_expert() const { return router == RouterForm::Fused || router == RouterForm::Split; }
};

// what plan_expert_ffn is asked for: fp8 arithmetic where the layer has a calibrated H scale
static ExpertWeights expert_weights(const m3_engine_config& c, const BlockW& w) {
  if (c.weight_dtype == M3_F32) return ExpertWeights::F32;
  if (c.weight_dtype == M3_BF16) return ExpertWeights::BF16;
  if (c.weight_dtype == M3_MXFP4) return ExpertWeights::MXFP4;
  return w.h_scale > 0.f ? ExpertWeights::FP8A8 : ExpertWeights::FP8;
}

MoeRoute choose_moe_route(const m3_engine_config& c, int S, const BlockW& w, const Plan& pl) {
  const Switches& sw = switches();
  const int world = c.ep_world_size > 0 ? c.ep_world_size : 1;
  const int E = c.num_experts, Etot = E * world, D = c.attention_dim, De = c.embed_dim, F = c.hidden_units;
  const bool one_wg_experts = Etot == 8 || Etot == 16 || Etot == 32 || Etot == 64;   // what the single-work-group kernels take
  // S <= 256 rows, all experts local, fp32: the expert launch can route for itself
  const bool self_routing = sw.self_route && c.weight_dtype == M3_F32 && expert_ffn_f32_self_routing(S, Etot) &&
                            plan_expert_ffn(ExpertWeights::F32, S, E, D, F).kernel == ExpertKernel::SlabF32;
  MoeRoute r;
  r.ep = world > 1 || c.ep_stages > 0;
  if (c.fuse_route == 2 && world == 1 && S < 1024 && one_wg_experts) {
    r.router = RouterForm::Split;
    r.gate = self_routing ? GateForm::InExpert : GateForm::GateIndex;
  } else if (c.fuse_route == 1 && world == 1 && S <= 256 && (E == 16 || E == 32 || E == 64)) {
    r.router = RouterForm::Fused;
    r.gate = GateForm::InRoute;
  } else {
    r.router = moe_router_supports(De, D, Etot) && S >= sw.router_min_rows ? RouterForm::Kernel : RouterForm::Gemm;
    r.router_top1 = r.router == RouterForm::Kernel && moe_router_fuses_top1(Etot) && S > sw.gate_index_max_rows;
    if (self_routing && c.fuse_route == 0 && !r.ep) r.gate = GateForm::InExpert;
    else if (S <= sw.gate_index_max_rows && one_wg_experts) r.gate = GateForm::GateIndex;
    else r.gate = r.router_top1 ? GateForm::RouterTail : GateForm::Top1Index;
  }
  const bool fused8 = !r.ep && plan_expert_ffn(expert_weights(c, w), S, E, D, F).kernel == ExpertKernel::FusedFp8;
  r.use_xq = r.router == RouterForm::Kernel && sw.router_xq && fused8 && pl.xq != nullptr;
  r.skip_xn = r.use_xq && sw.router_skip_xn && !c.debug_taps;
  r.fs_dev = sw.fused8_adapt && fused8 && pl.moe_fs != nullptr && !c.debug_taps;
  r.needs_e_all = r.norm_in_expert();
  return r;
}

// The staged router GEMM of a main block on cat([embed, x]): the operands every layer shares (add_moe_router adds the layer's)
GemmParams router_concat_gemm(const m3_engine_config& c, int S, const float* emb, const float* x) {
  const int world = c.ep_world_size > 0 ? c.ep_world_size : 1;
  const int D = c.attention_dim, De = c.embed_dim, Etot = c.num_experts * world;
  GemmParams g;
  g.ldy = Etot; g.M = S; g.N = Etot;
  g.mode = GEMM_A_CONCAT2; g.A = emb; g.lda = De; g.K1 = De; g.A2 = x; g.lda2 = D; g.K = De + D;
  g.ln_on_a2 = 1; g.ld_ln_out = D;
  return g;
}
// Floats per layer of the routers' accumulator prefix, 0 where it is not taken.  Taken (M3_ROUTER_PREFIX) by the staged fp32
// router of short inputs: S <= 128 rows -- the 16-row-tile regime, where the router's few work-groups each pull both halves
// through one CU; on long batches the prefix is as many bytes as the embed rows it saves -- and the GEMM planning as the form
// that takes acc_init (De = D = 256 or 512 today).
size_t router_prefix_layer_floats(const m3_engine_config& c, int S, const Plan& pl) {
  if (!switches().router_prefix || c.weight_dtype != M3_F32 || c.embed_dim < 256 || S > 128 || c.num_blocks < 1 ||
      c.num_blocks > kRouterPrefixMaxLayers)
    return 0;
  if (choose_moe_route(c, S, BlockW(), pl).router != RouterForm::Gemm) return 0;
  static const float some = 0.f;   // (plan_gemm asks which operands exist, not where)
  GemmParams g = router_concat_gemm(c, S, &some, &some);
  g.W = &some; g.Y = const_cast<float*>(&some); g.ln_gamma = g.ln_beta = &some; g.acc_init = &some;
  const GemmPlan plan = plan_gemm(g, 0);
  return plan.launches == 1 ? router_prefix_floats(plan) : 0;
}

// What the stage list of one binding is built with.  The binding under construction is a local of build_binding: the engine
// sees it only once it is complete (bind), so a build that fails leaves the engine as it was.
struct StageBuilder {
  const m3_engine& eng;     // weights, config
  Plan pl;                  // the buffer plan over the key's workspace (the main encoder's view; embed_view for the embed chain)
  m3_engine::Bound& bd;     // the binding under construction
  StreamState st;           // streaming keys: the caller-owned state, carved once
  // what one build_* call hands to the next:
  bool lens_in_conv1 = false;   // the next conv1 stage also forms the subsampled lengths
  const float *tail_ln_g = nullptr, *tail_ln_b = nullptr; float tail_ln_eps = 0.f; float* tail_ln_out = nullptr;   // a second LayerNorm for the next norm_final stage
  float* splitk_ws = nullptr; size_t splitk_bytes = 0;   // partial tiles of the split-K front-end GEMMs now being added (inside the workspace)
};

}  // namespace

// ------------------------------------------------------------------------------------------------
static void add_stage(StageBuilder& sb, const std::string& name, int kernels, std::function<int(hipStream_t)> fn,
                      m3_stage_info info = stage_info("", 0, 0.0, 0.0)) {
  info.launches = kernels;
  sb.bd.stages.push_back(Stage{name, std::move(fn), info});
  sb.bd.n_kernels += kernels;
}

// algorithmic traffic of one GEMM: weights once, A rows once, result once (+ the residual it adds, + side outputs)
static m3_stage_info gemm_info(const GemmParams& p, const GemmPlan& plan) {
  const bool glu = p.act == ACT_GLU;
  const double M = p.M, N = p.N, K = p.K, Nout = glu ? N / 2 : N;
  const double wsz = p.w_bf16 ? 2 : 4, asz = p.a_bf16 ? 2 : 4, ysz = p.y_bf16 ? 2 : 4;
  double a_bytes = M * K * asz;
  if (p.mode == GEMM_A_CONV3X3S2)   // implicit conv: the input tensor is read once, not 9 times
    a_bytes = (double)(p.M / (p.conv_T2 * p.conv_F2)) * p.conv_T1 * p.conv_F1 * p.conv_C * asz;
  double bytes = N * K * wsz + a_bytes + M * Nout * ysz;
  if (p.resid) bytes += M * Nout * 4;
  if (p.Yb) bytes += M * Nout * 2;
  if (p.ln_out) bytes += M * (K - p.K1) * 4;
  return stage_info(plan.label, 1, bytes, 2.0 * M * N * K, p.mode != GEMM_A_CONV3X3S2);
}

static void add_launch(StageBuilder& sb, const std::string& name, Launch record, const m3_stage_info& info, bool pairable = false) {
  add_stage(sb, name, info.launches, nullptr, info);
  sb.bd.stages.back().launch = std::move(record);
  sb.bd.stages.back().pairable = pairable;
}

// fp32_weights: the router GEMMs keep fp32 weights in every mode (a flipped top-1 is a discrete error)
// wfrag: p.W in fragment order (Lin::wf), read instead where the bound shape plans as the skinny fp32 form and the plan takes the
// layout -- the same form, instantiation and grid, only the weight addresses differ; every other form reads the row-major p.W
static void add_gemm(StageBuilder& sb, const std::string& name, GemmParams p, bool fp32_weights = false, const float* wfrag = nullptr) {
  p.w_bf16 = (!fp32_weights && sb.eng.cfg.weight_dtype != M3_F32) ? 1 : 0;
  // planned once, when the shape is bound: the stage runs the record made here (a plan no kernel takes fails there, with its reason)
  GemmLaunch g = gemm_launch(p, sb.splitk_ws, sb.splitk_bytes);
  if (wfrag != nullptr && g.plan.launches == 1 && g.plan.kernel == GemmKernel::SkinnyF32) {
    GemmParams q = p;
    q.W = wfrag; q.w_frag = 1;
    const GemmLaunch gf = gemm_launch(q, sb.splitk_ws, sb.splitk_bytes);
    if (gf.plan.launches == 1) g = gf;
  }
  m3_stage_info info = gemm_info(p, g.plan);
  info.launches = g.plan.launches ? g.plan.launches : 1;
  add_launch(sb, name, g, info, g.plan.launches == 1);   // (a split-K stage: build_subsample decides whether it may pair)
}

// Horizontal fusion (B = 1-sized fp32 plans): the embed encoder and the main encoder's prefix -- its subsampling and block 0 up to
// the router, the first stage that reads the embedding -- are two independent chains.  Where a stage of each is a skinny fp32
// GEMM of the same instantiation, the two become ONE launch (gemm_f32_dual_kernel): a launch saved is ~6 us of a forward that is
// 275 dependent launches.  Each chain keeps its own order; only the first embed stage (it also derives the output lengths every
// later kernel reads) is guaranteed to stay in front of every main-prefix stage.  Arithmetic per problem is unchanged: results
// are bit-identical.  M3_HFUSE=0: off.
static bool stages_fusable(const Stage& a, const Stage& b) {
  if (!a.pairable || !b.pairable || a.launch.index() != b.launch.index()) return false;
  if (std::holds_alternative<GemmLaunch>(a.launch))   // (one launch each, or split-K + reduce each)
    return is_splitk(a) ? gemm_splitk_dual_fusable(gemm_of(a), gemm_of(b)) : gemm_dual_fusable(gemm_of(a), gemm_of(b));
  if (auto* d = std::get_if<DwArgs>(&a.launch)) return dwconv_dual_fusable(*d, std::get<DwArgs>(b.launch));
  if (auto* t = std::get_if<AttArgs>(&a.launch)) return relpos_attention_dual_fusable(*t, std::get<AttArgs>(b.launch));
  return conv1_dual_fusable(std::get<Conv1Args>(a.launch), std::get<Conv1Args>(b.launch));
}
// The pair of two fusable stages as one closure stage (never pairable again), from the records the two would have run.
// (a split-K pair is two stages, the GEMM launch and the reduce launch -- `reduce_half`, named a.reduce+b.reduce: every stage
//  named a+b is one launch that replaces two)
static Stage fused_stage(const Stage& a, const Stage& b, bool reduce_half = false) {
  Stage d;
  d.name = reduce_half ? a.name + ".reduce+" + b.name + ".reduce" : a.name + "+" + b.name;
  const char* label = "";
  std::visit([&](const auto& pa) {
    using R = std::decay_t<decltype(pa)>;
    if constexpr (std::is_same_v<R, GemmLaunch>) {
      const GemmLaunch& pb = gemm_of(b);
      if (is_splitk(a)) {
        d.run = [pa, pb, which = reduce_half ? 2 : 1](hipStream_t s) { return launch_gemm_f32_splitk_dual(pa, pb, s, which); };
        label = "gemm_f32_splitk_dual_kernel";   // (both halves: the unpaired stage carries its reduce under the GEMM's label too)
      } else {
        d.run = [pa, pb](hipStream_t s) { return launch_gemm_f32_dual(pa, pb, s); };
        label = "gemm_f32_dual_kernel";
      }
    } else if constexpr (std::is_same_v<R, Conv1Args>) {
      d.run = [pa, pb = std::get<R>(b.launch)](hipStream_t s) { return launch_conv1_relu_dual(pa, pb, s); };
      label = "conv1_relu_dual_kernel";
    } else if constexpr (std::is_same_v<R, DwArgs>) {
      d.run = [pa, pb = std::get<R>(b.launch)](hipStream_t s) { return launch_dwconv_ln_silu_dual(pa, pb, s); };
      label = "dwconv_ln_silu_dual_kernel";
    } else if constexpr (std::is_same_v<R, AttArgs>) {
      d.run = [pa, pb = std::get<R>(b.launch)](hipStream_t s) { return launch_relpos_attention_dual(pa, pb, s); };
      label = "relpos_attention_dual_kernel";
    }
  }, a.launch);
  // (the algorithmic bytes and FLOPs of a split-K pair stand with its GEMM stage; the partial tiles are not algorithmic traffic)
  d.info = reduce_half ? stage_info(label, 1, 0.0, 0.0, a.info.per_row != 0)
                       : stage_info(label, 1, a.info.alg_bytes + b.info.alg_bytes, a.info.flops + b.info.flops, a.info.per_row != 0);
  return d;
}
static void fuse_independent_pairs(StageBuilder& sb, int first, int mid, int join) {
  if (first < 0 || mid <= first + 1 || join <= mid) return;
  std::vector<Stage>& st = sb.bd.stages;
  std::vector<Stage> out(st.begin(), st.begin() + first);
  std::vector<Stage> pending;                         // main-prefix stages waiting for the next pair they precede
  int i = first, saved = 0;
  for (int m = mid; m < join; ++m) {
    assert(!st[m].reads_embed);                       // (moved ahead of embed stages: must not need the embedding)
    int partner = -1;
    if (st[m].pairable)
      // (the first embed stage pairs only as the subsamplers' conv1: no main-prefix stage is then in front of it either)
      for (int k = std::holds_alternative<Conv1Args>(st[m].launch) ? i : std::max(i, first + 1); k < mid; ++k)
        if (stages_fusable(st[k], st[m])) { partner = k; break; }
    if (partner < 0) { pending.push_back(st[m]); continue; }
    for (; i < partner; ++i) out.push_back(st[i]);
    for (Stage& q : pending) out.push_back(q);
    pending.clear();
    out.push_back(fused_stage(st[partner], st[m]));
    saved += st[partner].info.launches + st[m].info.launches - 1;
    if (is_splitk(st[m])) {
      out.push_back(fused_stage(st[partner], st[m], true));
      saved -= 1;
    }
    i = partner + 1;
  }
  for (; i < mid; ++i) out.push_back(st[i]);
  for (Stage& q : pending) out.push_back(q);
  for (int k = join; k < (int)st.size(); ++k) out.push_back(st[k]);
  st.swap(out);
  sb.bd.n_kernels -= saved;
}

// the first stage from `from` on that reads the embedding: where the main encoder joins the embed encoder (-1: none).  The forked
// capture runs [main start, join) beside the embed chain, horizontal fusion interleaves the two.
static int embed_join(const std::vector<Stage>& st, int from) {
  for (int i = from; i < (int)st.size(); ++i)
    if (st[i].reads_embed) return i;
  return -1;
}

static void build_subsample(StageBuilder& sb, const std::string& pfx, const SubW& w, int D, const Plan& pl, float* xout) {
  const m3_engine_config& c = sb.eng.cfg;
  const int B = sb.bd.key.B, T = sb.bd.key.T;
  const int fc = sub_fc(c.input_dim, w.in_ch);   // bins per input channel of this encoder's first conv
  const int T1 = (T - 3) / 2 + 1, F1 = sub_f1(fc), F2 = sub_f2(fc), T2 = (T1 - 3) / 2 + 1;
  const float* feat = sb.bd.key.feat;
  float* c1 = pl.c1; float* c2 = pl.c2;
  const int idim = c.input_dim;
  const float* cm = sb.eng.cmvn_mean; const float* ci = sb.eng.cmvn_istd;
  const bool a16 = sb.bd.a16;    // c1, c2 only feed GEMMs: kept as bf16; the Linear also writes the bf16 copy of x
  // (the forward's first conv1 also forms the subsampled lengths when no stage in front of it needs them: see "lens" below)
  const int32_t* flen = sb.lens_in_conv1 ? sb.bd.key.feat_len : nullptr;
  int32_t* lens_out = pl.lens;
  sb.lens_in_conv1 = false;
  Conv1Args ca;
  ca.feat = feat; ca.w9c = w.c1w; ca.bias = w.c1b; ca.cmvn_mean = cm; ca.cmvn_istd = ci; ca.B = B; ca.T = T; ca.idim = idim; ca.C = D; ca.out = c1;
  ca.relu = 1; ca.out_bf16 = a16; ca.feat_len = flen; ca.lens_out = lens_out; ca.in_ch = w.in_ch;
  add_launch(sb, pfx + "conv1", ca,
             stage_info("conv1_relu_kernel", 1, (double)B * T * idim * 4 + (double)B * T1 * F1 * D * (a16 ? 2 : 4), 18.0 * w.in_ch * B * T1 * F1 * D, false));
  const size_t conv1_at = sb.bd.stages.size() - 1;
  GemmParams g;
  g.a_bf16 = a16; g.y_bf16 = a16;
  g.mode = GEMM_A_CONV3X3S2; g.A = c1; g.lda = 4;
  g.conv_T1 = T1; g.conv_F1 = F1; g.conv_T2 = T2; g.conv_F2 = F2; g.conv_C = D;
  g.W = w.c2w; g.bias = w.c2b; g.Y = c2; g.ldy = D; g.M = B * T2 * F2; g.N = D; g.K = 9 * D; g.act = ACT_RELU;
  if (sb.bd.packed) g.conv_len = pl.lens;   // tiles of padded frames only: skipped (never gathered into the packed rows)
  add_gemm(sb, pfx + "conv2", g);
  // The front-end stages may share launches with the other subsampler's (fuse_independent_pairs) where this conv2 is a split-K
  // problem (C >= 512): below that the launches are short, and the stage lists of the small models stay what they were.
  auto splitk_with_ws = [&] { return is_splitk(sb.bd.stages.back()) && gemm_of(sb.bd.stages.back()).ws != nullptr; };
  const bool pairable = switches().front_pair && !a16 && !sb.bd.packed && splitk_with_ws();
  if (pairable) sb.bd.stages[conv1_at].pairable = sb.bd.stages.back().pairable = true;
  // Linear(C*F2 -> D) on the (f, c)-ordered flatten, with the positional-encoding scale sqrt(D)
  // (rel_positional_encoding_kernel.cu:62-69) folded into the epilogue.
  // packed ragged batch: the subsampler works on the padded (B, T) input; its rows are packed right after it
  const bool packed = sb.bd.packed;
  GemmParams l;
  l.A = c2; l.lda = F2 * D; l.W = w.out.w; l.bias = w.out.b; l.Y = packed ? pl.xpad : xout; l.ldy = D;
  l.M = B * T2; l.N = D; l.K = F2 * D; l.alpha = sqrtf((float)D);
  l.a_bf16 = a16;
  if (a16) { l.Yb = packed ? pl.xbpad : pl.xb; l.ldyb = D; }
  add_gemm(sb, pfx + "linear", l);
  if (pairable && splitk_with_ws()) sb.bd.stages.back().pairable = true;
  if (packed) {
    const float* xpad = pl.xpad; const void* xbpad = pl.xbpad; void* xb = pl.xb; const int32_t* pad_of = pl.pad_of;
    const int S = B * T2;
    add_stage(sb, pfx + "pack", a16 ? 2 : 1, [=](hipStream_t s) {
      if (int rc = launch_local_gather(xpad, pad_of, S, D * 4, xout, s)) return rc;
      return a16 ? launch_local_gather(xbpad, pad_of, S, D * 2, xb, s) : 0;
    }, stage_info("row_permute_kernel", 1, (double)S * D * (a16 ? 12 : 8) + 4.0 * S, 0.0));
  }
  if (sb.bd.dma) {   // the first block's folded-LayerNorm GEMM takes the row statistics of xb from its producer: here a pass of its own
    const void* xbv = pl.xb; float* xs = pl.xstats;
    const int S = B * T2;
    add_stage(sb, pfx + "row_stats", 1, [=](hipStream_t s) { return launch_row_stats_bf16(xbv, S, D, xs, s); },
              stage_info("row_stats_bf16_kernel", 1, (double)S * D * 2 + 32.0 * S, 3.0 * S * D));
  }
}

// ---- the MoE half of a main block: the stages of one route (choose_moe_route), one builder per stage kind ----
// What the MoE stages of one layer work on
struct MoeLayer {
  std::string pfx;
  const BlockW* w;
  int S, Tp, D, F, De, E, Etot, world;   // E local experts, Etot = E * world router outputs
  float eps;
  float *x, *xn, *rl;
  int32_t* gidx; float* gval;
  const float* gv;                       // gate values the combine scales by (null: keep_expert_output)
  const int32_t *lens, *live_len; int live_rpb;   // which rows are padding (padded or packed layout)
  const int32_t* pdev;                   // packed rows: the live-row count on the device (else null)
  const float* eall; int ld_eall;        // this layer's columns of router_e_all's output
  int layer;                             // index among the main blocks
  void* xb_out; float* xstats_out;       // 16-bit modes: the combine also writes the bf16 copy of x / its row statistics
  void* ws; MoeWorkspace mw;             // the layer's MoE workspace, carved for the S local rows
};

static void add_moe_router(StageBuilder& sb, const MoeLayer& m, const MoeRoute& r, const Plan& pl) {
  const BlockW& w = *m.w;
  const int S = m.S, D = m.D, De = m.De, E = m.E, Etot = m.Etot;
  if (r.router == RouterForm::Fused) {
    add_stage(sb, m.pfx + "moe_route", 1, [m](hipStream_t s) {
      const BlockW& w = *m.w;
      return launch_moe_route(m.x, m.D, m.D, w.router_x.w, w.router_x.wsum, w.router_x.b, m.eall, m.ld_eall, m.eps, m.lens, m.Tp,
                              m.S, m.E, m.gidx, m.gval, m.mw.mapping, m.mw.acc, m.mw.pos, s);
    }, stage_info("moe_route_kernel", 1, (double)E * D * 4 + (double)S * (D + E) * 4 + 16.0 * S, 2.0 * S * E * D));
  } else if (r.router == RouterForm::Kernel) {
    void* xq = r.use_xq ? pl.xq : nullptr; float* xqs = r.use_xq ? pl.xq_scale : nullptr;
    float* xn_out = r.skip_xn ? nullptr : m.xn;
    if (r.skip_xn) sb.bd.xn_skipped = true;   // ("xn" is then not offered as a buffer: a reader fails instead of reading stale rows)
    int32_t* gidx = r.router_top1 ? m.gidx : nullptr; float* gval = r.router_top1 ? m.gval : nullptr;
    const float* emb = pl.emb;
    add_stage(sb, m.pfx + "moe_router", 1, [=](hipStream_t s) {
      const BlockW& w = *m.w;
      return launch_moe_router(emb, m.De, m.De, m.x, m.D, m.D, w.router.w, w.router.b, w.n_ff.g, w.n_ff.b, m.eps, xn_out, m.D, m.rl,
                               m.Etot, m.S, m.Etot, m.pdev, s, gidx, gval, m.live_len, m.live_rpb, xq, xqs);
    }, stage_info("moe_router_kernel", 1, (double)Etot * (De + D) * 4 + (double)S * (De + 2 * D + Etot) * 4, 2.0 * S * Etot * (De + D)));
  } else {
    GemmParams g;
    g.Y = m.rl; g.ldy = Etot; g.M = S; g.N = Etot; g.m_dev = m.pdev;
    if (r.router == RouterForm::Split) {   // norm_ff folded into the x-half weight (output-side LayerNorm), embed half as residual
      g.A = m.x; g.lda = D; g.W = w.router_x.w; g.bias = w.router_x.b; g.ln_wsum = w.router_x.wsum; g.ln_eps = m.eps; g.K = D;
      g.resid = m.eall; g.ldr = m.ld_eall;
    } else {   // LayerNorm(norm_ff) on the x half of cat([embed, x]) as the prologue, written out once as xn (the expert FFN's input)
      g = router_concat_gemm(sb.eng.cfg, S, pl.emb, m.x);
      g.Y = m.rl; g.m_dev = m.pdev;
      g.W = w.router.w; g.bias = w.router.b;
      g.ln_gamma = w.n_ff.g; g.ln_beta = w.n_ff.b; g.ln_eps = m.eps; g.ln_out = m.xn;
      // the embed half was run by "router_e_prefix": the waves start from its accumulators and walk the x half only
      if (pl.rprefix != nullptr) g.acc_init = pl.rprefix + (size_t)m.layer * pl.rprefix_layer;
    }
    add_gemm(sb, m.pfx + "moe_router", g, true);
    if (g.acc_init != nullptr) {
      Stage& st = sb.bd.stages.back();
      // (what moved to the prefix stage: the embed rows, the embed columns of the weight, their FLOPs; what came: the prefix read)
      st.info.alg_bytes += 4.0 * pl.rprefix_layer - 4.0 * De * (Etot + S);
      st.info.flops -= 2.0 * S * Etot * De;
      const GemmPlan plan = gemm_of(st).plan;
      float* prefix = pl.rprefix; const int layer = m.layer;
      st.refresh_prefix = [plan, g, prefix, layer](hipStream_t s) {
        const float* wt[kRouterPrefixMaxLayers] = {};
        wt[layer] = g.W;
        return launch_router_embed_prefix(plan, g, wt, layer, 1, prefix, s);
      };
    }
  }
  sb.bd.stages.back().reads_embed = true;
}

// SoftmaxTopK plugin + ScatterMapping kernel of the reference in ONE launch (a single work-group: right for a few hundred rows);
// the index over the local (map, acc, pos) or, expert parallel, over the global expert ids
static void add_moe_gate_index(StageBuilder& sb, const MoeLayer& m, int32_t* map, int32_t* acc, int32_t* pos) {
  add_stage(sb, m.pfx + "moe_gate_index", 1, [=](hipStream_t s) {
    return launch_moe_gate_index(m.rl, m.Etot, m.live_len, m.live_rpb, m.S, m.gidx, m.gval, map, acc, pos, s);
  }, stage_info("moe_index_kernel", 1, (double)m.S * (m.Etot * 4 + 16) + 4.0 * (m.Etot + 1), 0.0));
}

static void add_moe_top1(StageBuilder& sb, const MoeLayer& m) {
  add_stage(sb, m.pfx + "moe_top1", 1, [m](hipStream_t s) {
    return launch_softmax_top1(m.rl, m.Etot, m.live_len, m.live_rpb, m.S, m.Etot, m.gidx, m.gval, s);
  }, stage_info("softmax_top1_kernel", 1, (double)m.S * (m.Etot * 4 + 8), 0.0));
}

static void add_moe_local_index(StageBuilder& sb, const MoeLayer& m) {
  add_stage(sb, m.pfx + "moe_local.index", 1, [m](hipStream_t s) {
    return launch_moe_index(m.gidx, m.S, m.E, m.mw.mapping, m.mw.acc, m.mw.pos, s);
  }, stage_info("moe_index_kernel", 1, 12.0 * m.S + 4.0 * (m.E + 1), 0.0));
}

// the plan's arguments on the R rows of x that (mw.pos, mw.acc) sort by expert; the result goes into mw.slab
static ExpertFfnArgs expert_args(const BlockW& w, const float* x, const MoeWorkspace& mw, int D) {
  ExpertFfnArgs a{};
  a.x = x; a.ldx = D; a.pos = mw.pos; a.acc_hist = mw.acc; a.w1 = w.ew1; a.w2 = w.ew2; a.s1 = w.es1; a.s2 = w.es2; a.b1 = w.eb1;
  a.w2_sliced = EXPERT_W2_SLICED; a.h_scale = w.h_scale; a.slab = mw.slab;
  return a;
}

static void add_moe_local_expert(StageBuilder& sb, const MoeLayer& m, const MoeRoute& r, const ExpertFfnPlan& f, const Plan& pl) {
  const bool norm = r.norm_in_expert();
  const float* xin = norm ? m.x : m.xn;
  const bool self_route = r.gate == GateForm::InExpert;
  const void* xq = r.use_xq ? pl.xq : nullptr; const float* xqs = r.use_xq ? pl.xq_scale : nullptr;
  int32_t* fs = r.fs_dev ? pl.moe_fs : nullptr;
  add_stage(sb, m.pfx + "moe_local.expert", f.launches, [=](hipStream_t s) {
    const BlockW& w = *m.w;
    const float* ln_g = norm ? w.n_ff.g : nullptr; const float* ln_b = norm ? w.n_ff.b : nullptr; const float ln_eps = norm ? m.eps : 0.f;
    // short inputs, fp32: SoftmaxTopK + ScatterMapping happen inside the expert launch (every work-group derives its expert's
    // rows from the router logits; moe_expert.hip "self-routing form"); its slabs hold ORIGINAL rows, b2 inside
    const bool wf = w.ew1f != nullptr;   // (fp32 experts in fragment order: the one-launch kernel's two forms read them)
    if (self_route)
      return launch_expert_route_ffn_f32(xin, m.D, m.rl, m.live_len, m.live_rpb, m.S, m.E, m.D, m.F, wf ? w.ew1f : w.ew1, w.eb1,
                                         wf ? w.ew2f : w.ew2, wf ? EXPERT_W_FRAG : EXPERT_W2_SLICED, w.eb2, m.mw.slab, m.gidx, m.gval, m.mw.mapping, m.mw.acc, m.mw.pos, s, ln_g, ln_b, ln_eps);
    ExpertFfnArgs a = expert_args(w, xin, m.mw, m.D);
    a.ln_gamma = ln_g; a.ln_beta = ln_b; a.ln_eps = ln_eps; a.xq = xq; a.xq_scale = xqs; a.fs_dev = fs;
    if (wf && f.kernel == ExpertKernel::SlabF32) { a.w1 = w.ew1f; a.w2 = w.ew2f; a.w2_sliced = EXPERT_W_FRAG; }
    return launch_expert_ffn(f, m.S, m.E, m.D, m.F, a, s);
  }, stage_info(f.label, 1, -1.0, 4.0 * m.D * m.F * m.S));
}

// local_gather + b2 + gate + residual + LayerNorm(norm_final) over the expert outputs
static void add_moe_local_combine(StageBuilder& sb, const MoeLayer& m, const MoeRoute& r, const ExpertFfnPlan& f, const Plan& pl) {
  // (self-routing expert launch: slabs hold ORIGINAL rows with b2 already in slice 0 -> no mapping, no b2 here)
  const bool self_route = r.gate == GateForm::InExpert;
  const int32_t* cmap = self_route ? nullptr : m.mw.mapping;
  const float* cb2 = self_route ? nullptr : m.w->eb2;
  const int32_t* fs = r.fs_dev ? pl.moe_fs : nullptr;
  const double S = m.S, D = m.D;
  add_stage(sb, m.pfx + "moe_local.combine", 1, [=](hipStream_t s) {
    const BlockW& w = *m.w;
    return launch_moe_combine(f.rows(m.mw.slab), fs ? kExpertFusedFp8MaxSplit : f.slices, cmap, m.gidx, m.gv, cb2, m.x, 0.5f, w.n_final.g, w.n_final.b, m.eps, m.x,
                              m.S, m.D, s, m.xb_out, m.xstats_out, fs);
  }, stage_info("moe_combine_kernel", 1, S * D * 4 * (f.slices + 2) + (m.xb_out ? 2.0 * S * D : 0.0), S * D * (f.slices + 10)));
}

// Expert parallel (m3asr/ep.py drives the two all-to-alls between these stages; FastMoE semantics
// trainer_3m_fix/fmoe/functions.py:13-86,175-199): nothing returns to the host, the exchange has a fixed shape
// wire [world][1 + C][D]: chunk j = what goes to / came from rank j, header row = E_loc row counts
static void add_moe_ep(StageBuilder& sb, const MoeLayer& m, const MoeRoute& r, const Plan& pl) {
  const int S = m.S, E = m.E, Etot = m.Etot, D = m.D, F = m.F, world = m.world;
  const int cap = pl.ep_cap, R = pl.ep_rows;
  int32_t *g_acc = pl.ep_acc, *g_map = pl.ep_mapping, *g_pos = pl.ep_pos, *map_send = pl.ep_map_send, *gate_recv = pl.ep_gate_recv;
  int32_t* ep_overflow = pl.ep_overflow;
  float *wire_a = pl.wire_a, *wire_b = pl.wire_b;
  const MoeWorkspace rw = carve_moe_workspace(m.ws, R, E, D, F);     // receive side: R wire rows over the E local experts
  // top-1 + index over GLOBAL expert ids (the same kernel choice by row count as with all experts local)
  if (r.gate == GateForm::GateIndex) add_moe_gate_index(sb, m, g_map, g_acc, g_pos);
  if (r.gate == GateForm::Top1Index) add_moe_top1(sb, m);
  // wire row of every token (+ count headers), rows scattered straight into the send wire
  const bool one_launch = r.gate == GateForm::GateIndex;
  const int32_t* gidx = m.gidx; const float* xn = m.xn;
  add_stage(sb, m.pfx + "moe_ep.send", one_launch ? 1 : 2, [=](hipStream_t s) {
    if (!one_launch)
      if (int rc = launch_moe_index(gidx, S, Etot, g_map, g_acc, g_pos, s)) return rc;
    return launch_ep_send_rows(gidx, g_map, g_acc, S, world, E, cap, map_send, xn, wire_a, D * 4, s, ep_overflow);
  }, stage_info("ep_send_rows_kernel", 1, (double)S * D * 8 + 24.0 * S, 0.0));
  auto exchange = [=, &sb](const char* name) {   // one rank: the all-to-all is a copy
    if (world == 1) add_stage(sb, m.pfx + name, 0, [=](hipStream_t s) {
      M3_CHECK_HIP(hipMemcpyAsync(wire_b, wire_a, (size_t)R * D * 4, hipMemcpyDeviceToDevice, s));
      return 0;
    });
  };
  exchange("moe_ep.exchange1");
  // this rank's experts on everything it received (its own stable index puts the rows in FastMoE's receive order: by local
  // expert, then source rank, then wire order); results return to wire_a at the wire rows they came in on
  const ExpertFfnPlan f = plan_expert_ffn(expert_weights(sb.eng.cfg, *m.w), R, E, D, F, EXPERT_SCATTER_ROWS);
  // bf16 experts in the tiled two-GEMM form: GEMM-2's epilogue adds b2 and puts every row straight back on its wire row
  // (no un-permuting combine launch; wire rows nobody sent keep stale bytes -- no rank ever reads them back)
  const bool scatter2 = f.kernel == ExpertKernel::TiledBf16;
  const BlockW* wp = m.w;
  add_stage(sb, m.pfx + "moe_ep.expert", (scatter2 ? 2 : 3) + f.launches, [=](hipStream_t s) {
    const BlockW& w = *wp;
    if (int rc = launch_ep_recv_gate(wire_b, world, E, cap, D * 4, gate_recv, s)) return rc;
    if (int rc = launch_moe_index(gate_recv, R, E, rw.mapping, rw.acc, rw.pos, s)) return rc;
    ExpertFfnArgs a = expert_args(w, wire_b, rw, D);
    if (scatter2) { a.b2 = w.eb2; a.y_scatter = wire_a; }
    if (int rc = launch_expert_ffn(f, R, E, D, F, a, s)) return rc;
    if (scatter2) return 0;
    return launch_moe_combine(f.rows(rw.slab), f.slices, rw.mapping, gate_recv, nullptr, w.eb2, nullptr, 1.f, nullptr, nullptr, 0.f, wire_a, R, D, s);
  }, stage_info(f.label, 1, -1.0, 4.0 * D * F * S));
  exchange("moe_ep.exchange2");
  // local_gather + gate + residual + LayerNorm: token s reads its result at the wire row it was sent from
  add_stage(sb, m.pfx + "moe_ep.combine", 1, [=](hipStream_t s) {
    const BlockW& w = *wp;
    return launch_moe_combine(wire_b, 1, map_send, nullptr, m.gv, nullptr, m.x, 0.5f, w.n_final.g, w.n_final.b, m.eps, m.x, S, D, s,
                              m.xb_out, m.xstats_out);
  }, stage_info("moe_combine_kernel", 1, (double)S * D * 12 + (m.xb_out ? 2.0 * S * D : 0.0), (double)S * D * 11));
  sb.bd.buffers["ep.wire_a"] = Buf{wire_a, (size_t)R * D * 4};
  sb.bd.buffers["ep.wire_b"] = Buf{wire_b, (size_t)R * D * 4};
}

static void build_block(StageBuilder& sb, const std::string& pfx, const BlockW& w, int D, int F, int H, int K, bool cnn_ln,
                        bool moe, int layer, int tap_index, const Plan& pl, bool causal) {
  // every GEMM of a block is row-wise over the S rows of the batch: packed batches pass the live-row count
  auto add_gemm = [&](StageBuilder&, const std::string& name, GemmParams g, bool fp32_weights = false, const float* wfrag = nullptr) {
    if (sb.bd.packed) g.m_dev = pl.row0 + sb.bd.key.B;
    ::add_gemm(sb, name, g, fp32_weights, wfrag);
  };
  const m3_engine_config& c = sb.eng.cfg;
  const BindKey& key = sb.bd.key;
  const int B = key.B, Tp = sb.bd.Tp, S = sb.bd.S;
  // chunk-by-chunk binding: the chunk counter the attention core and the depthwise conv read.  Slot mode: the counter of
  // utterance b is slot_pos[b]; max_frames / c chunks fit (the kernels test a slot against it)
  const bool streaming = key.sstate != nullptr;
  const int32_t* step = key.s_slots ? sb.st.slot_pos : sb.st.step;
  const int slot_chunks = key.s_slots ? key.s_maxf / Tp : -1;
  float* x = pl.x;
  const int32_t* lens = pl.lens;
  const float eps = 1e-12f;  // all block LayerNorms (fmoe_transformer.py:54-65)

  // 16-bit modes, long batches: GEMM A operands come as bf16 -- the copy xb of the residual stream (written by every
  // kernel that writes x) and bf16 h1 / ctx / dw -- because these GEMMs are bound by the traffic of their fp32 A operand
  const bool a16 = sb.bd.a16;
  void* xb = pl.xb;
  const bool dma = sb.bd.dma;
  float* xstats = pl.xstats;
  auto from_xb = [&](GemmParams& g) {
    if (a16) { g.A = (const float*)xb; g.a_bf16 = 1; }
    if (dma) { g.ln_stats = xstats; g.ln_stat_parts = kXbStatParts; }
  };
  auto also_xb = [&](GemmParams& g) {
    if (a16) { g.Yb = xb; g.ldyb = D; }
    if (dma) g.Yb_stats = xstats;
  };
  // packed ragged batch: rows [0, P) are the valid frames of all utterances back to back, P = row0[B] on the device;
  // row-wise kernels skip the tiles beyond P, attention and the depthwise conv find their utterance through row0 / pad_of
  const bool packed = sb.bd.packed;
  const int32_t* row0 = packed ? pl.row0 : nullptr;
  const int32_t* pad_of = packed ? pl.pad_of : nullptr;
  const int32_t* pdev = packed ? pl.row0 + B : nullptr;
  // "frame t of utterance b is padding" for the gate: padded layout (lens, T'), packed layout one run of P rows
  const int32_t* live_len = packed ? pdev : lens;
  const int live_rpb = packed ? S : Tp;
  {  // x += 0.5 * FFN_macaron(LN(x))
    GemmParams g;
    g.A = x; g.lda = D; g.W = w.mac1.w; g.bias = w.mac1.b; g.Y = pl.h1; g.ldy = F; g.M = S; g.N = F; g.K = D;
    g.ln_wsum = w.mac1.wsum; g.ln_eps = eps; g.act = ACT_SILU;   // norm_ff_macaron is folded into w_1 (plan.py)
    from_xb(g); g.y_bf16 = a16;
    add_gemm(sb, pfx + "ffn_macaron.w1", g, false, w.mac1.wf);
    GemmParams h;
    h.A = pl.h1; h.lda = F; h.W = w.mac2.w; h.bias = w.mac2.b; h.Y = x; h.ldy = D; h.M = S; h.N = D; h.K = F;
    h.alpha = 0.5f; h.resid = x; h.ldr = D;
    h.a_bf16 = a16; also_xb(h);
    add_gemm(sb, pfx + "ffn_macaron.w2", h, false, w.mac2.wf);
  }
  {  // x += MHA(LN(x))
    GemmParams g;
    g.A = x; g.lda = D; g.W = w.qkv.w; g.bias = w.qkv.b; g.Y = pl.qkv; g.ldy = 3 * D; g.M = S; g.N = 3 * D; g.K = D;
    g.ln_wsum = w.qkv.wsum; g.ln_eps = eps;                  // norm_mha is folded into the qkv weight
    from_xb(g);
    // 16-bit modes, long batches, T' <= 128: q | k | v are written as bf16 and the attention core runs on bf16 MFMAs with
    // K / P / V of a head staged once per (utterance, head) (attention.hip, second kernel)
    const bool att16 = a16 && relpos_attention_bf16_supports(Tp, D / H);
    g.y_bf16 = att16;
    add_gemm(sb, pfx + "att.qkv", g, false, w.qkv.wf);
    // p = linear_pos(pos_emb) of all blocks comes from ONE GEMM per forward ("pos_all" stage):
    // block i's slice is columns [i*D, (i+1)*D) of pbuf [T'][n_blocks*D]
    const int ldp = (c.num_blocks + c.embed_blocks) * D;
    const float* pmat = pl.pbuf + (size_t)tap_index * D;
    const float* qkv = pl.qkv; float* ctx = pl.ctx;
    const float* pu = w.pos_u; const float* pv = w.pos_v;
    const int dk = D / H;
    const float scale = 1.f / sqrtf((float)dk);
    const int chunk = c.static_chunk_size, left_chunks = c.num_left_chunks;   // static chunk mask (0 = full context)
    AttArgs aa;
    aa.qkv = qkv; aa.ldq = 3 * D; aa.pmat = pmat; aa.ldp = ldp; aa.pos_u = pu; aa.pos_v = pv; aa.row_len = lens; aa.B = B; aa.T = Tp; aa.H = H;
    aa.dk = dk; aa.scale = scale; aa.out = ctx; aa.ldo = D; aa.left_chunks = left_chunks;
    const char* label = att16 ? "relpos_attention_bf16_kernel" : "relpos_attention_kernel";
    double row_bytes = att16 ? 8 : (12 + (a16 ? 2 : 4));
    if (streaming) {   // chunk-by-chunk: keys = K / V history + this chunk, positions absolute, history appended in place
      aa.streaming = 1; aa.hist = sb.st.kv[tap_index]; aa.cap = key.s_hist; aa.step = step; aa.slot_max_chunks = slot_chunks;
      label = "relpos_attention_stream_kernel"; row_bytes = 24;
    } else {
      aa.rows_bf16 = att16; aa.out_bf16 = a16; aa.row0 = row0; aa.chunk = chunk;
    }
    // (pairable: the fp32 core is a candidate for sharing a launch with the other encoder's, fuse_independent_pairs)
    add_launch(sb, pfx + "att.core", aa, stage_info(label, 1, (double)S * D * row_bytes + (double)Tp * D * 4, 6.0 * Tp * D * S), !streaming && !att16);
    GemmParams o;
    o.A = pl.ctx; o.lda = D; o.W = w.out.w; o.bias = w.out.b; o.Y = x; o.ldy = D; o.M = S; o.N = D; o.K = D;
    o.resid = x; o.ldr = D;
    o.a_bf16 = a16; also_xb(o);
    add_gemm(sb, pfx + "att.out", o, false, w.out.wf);
  }
  {  // x += ConvModule(LN(x))
    GemmParams g;
    g.A = x; g.lda = D; g.W = w.pw1.w; g.bias = w.pw1.b; g.Y = pl.glu; g.ldy = D; g.M = S; g.N = 2 * D; g.K = D;
    g.ln_wsum = w.pw1.wsum; g.ln_wbeta = w.pw1.wbeta; g.ln_eps = eps; g.act = ACT_GLU;   // norm_conv folded into pw1
    // padded frames enter the conv module as zeros (convolution.py:101-104); packed: the rows >= P are "padding", and
    // row P thereby receives the constant a zeroed frame produces -- the depthwise conv reads it for taps len <= t < T'
    g.row_len = live_len; g.rows_per_batch = live_rpb; g.mask_in = 1;
    from_xb(g);
    // GLU deferred to the depthwise kernel: pw1 as the plain one-column-tile form writing value | gate columns [S][2 D] (each
    // element what the GLU epilogue holds just before its GLU line), the depthwise kernel forms value * sigmoid(gate) per tap.
    // Same operations on the same operands: bit-identical.  Taken where a work-group's operand pull is what the launch costs
    // (16-row tiles, D >= 256); everywhere else the stage list is what it was.
    bool glu_deferred = false;
    if (switches().glu_defer && c.weight_dtype == M3_F32 && !a16 && !causal && !streaming &&
        dwconv_glu_in_supports(D, K, false, 0, 2 * D)) {
      GemmParams r = g;
      r.act = ACT_NONE; r.ldy = 2 * D;
      const GemmPlan rp = plan_gemm(r, 0);
      if (rp.launches == 1 && rp.kernel == GemmKernel::SkinnyF32 && rp.mt == 1) { g = r; glu_deferred = true; }
    }
    // ... and the gate's sigmoid taken where each gate element exists once, in pw1's epilogue (M3_GLU_SIG_EPI): the depthwise
    // kernel's taps are then one multiply each
    const bool glu_sig = glu_deferred && switches().glu_sig_epi && (D & 15) == 0;
    if (glu_sig) g.sig_col0 = D;
    add_gemm(sb, pfx + "conv.pw1_glu", g, false, w.pw1.wf);
    const float* glu = pl.glu; float* dw = pl.dw;
    const float* dww = w.dw_w; const float* dwb = w.dw_b;
    const float* ng = cnn_ln ? w.n_cnn.g : nullptr; const float* nb = cnn_ln ? w.n_cnn.b : nullptr;
    const float* lfill = causal ? w.left_fill : nullptr;   // causal conv module (convolution.py:43-49,118-123)
    DwArgs da;
    da.z = glu; da.w_kc = dww; da.bias = dwb; da.gamma = ng; da.beta = nb; da.eps = 1e-5f; da.B = B; da.T = Tp; da.D = D; da.K = K;
    da.out = dw; da.out_bf16 = a16;
    double row_bytes = (glu_deferred ? 8 : 4) + (a16 ? 2 : 4), cache_bytes = 0.0;
    if (streaming) {
      da.streaming = 1; da.cache_pair = sb.st.conv[tap_index]; da.step = step; da.chunk_len = lens; da.slot_max_chunks = slot_chunks;
      row_bytes = 8; cache_bytes = 8.0 * B * (K - 1) * D;
    } else {
      da.pad_of = pad_of; da.row0 = row0; da.row_len = lens; da.causal_left_fill = lfill;
      da.glu_ldz = glu_deferred ? 2 * D : 0; da.glu_sig = glu_sig;
    }
    add_launch(sb, pfx + "conv.dw_ln_silu", da,
               stage_info("dwconv_ln_silu_kernel", 1, (double)S * D * row_bytes + (double)K * D * 4 + cache_bytes, 2.0 * K * D * S), !streaming);
    GemmParams h;
    h.A = pl.dw; h.lda = D; h.W = w.pw2.w; h.bias = w.pw2.b; h.Y = x; h.ldy = D; h.M = S; h.N = D; h.K = D;
    h.row_len = live_len; h.rows_per_batch = live_rpb; h.mask_out = 1; h.resid = x; h.ldr = D;
    h.a_bf16 = a16; also_xb(h);
    add_gemm(sb, pfx + "conv.pw2", h, false, w.pw2.wf);
  }
  if (!moe) {  // x = LN_final(x + 0.5 * FFN(LN(x)))
    GemmParams g;
    g.A = x; g.lda = D; g.W = w.ff1.w; g.bias = w.ff1.b; g.Y = pl.h1; g.ldy = F; g.M = S; g.N = F; g.K = D;
    g.ln_wsum = w.ff1.wsum; g.ln_eps = eps; g.act = ACT_SILU;   // norm_ff is folded into w_1
    from_xb(g); g.y_bf16 = a16;
    add_gemm(sb, pfx + "ffn.w1", g, false, w.ff1.wf);
    GemmParams h;
    h.A = pl.h1; h.lda = F; h.W = w.ff2.w; h.bias = w.ff2.b; h.Y = x; h.ldy = D; h.M = S; h.N = D; h.K = F;
    h.alpha = 0.5f; h.resid = x; h.ldr = D;
    h.a_bf16 = a16;                                   // (x is rewritten by norm_final below: no bf16 copy here)
    add_gemm(sb, pfx + "ffn.w2", h, false, w.ff2.wf);
    const float* fg = w.n_final.g; const float* fb = w.n_final.b;
    void* xbo = a16 ? xb : nullptr;
    float* xso = dma ? xstats : nullptr;
    // (the embed encoder's last block: after_norm rides in the same launch, conformer_embed_domain_acc.py:171-181)
    const float* g2 = sb.tail_ln_g; const float* b2 = sb.tail_ln_b; float* y2 = sb.tail_ln_out;
    const float eps2 = sb.tail_ln_eps;
    sb.tail_ln_g = nullptr;
    add_stage(sb, pfx + "norm_final", 1, [=](hipStream_t s) { return launch_layernorm(x, fg, fb, eps, x, S, D, s, xbo, xso, g2, b2, eps2, y2); },
              stage_info("layernorm_kernel", 1, (double)S * D * (a16 ? 10 : 8) + (g2 ? 4.0 * S * D : 0.0), (g2 ? 16.0 : 8.0) * S * D));
  } else {  // x = LN_final(x + 0.5 * gate * Expert_g(LN(x)))     (positionwise_feed_forward.py:209-265)
    MoeLayer m;
    m.pfx = pfx; m.w = &w; m.S = S; m.Tp = Tp; m.D = D; m.F = F; m.De = c.embed_dim; m.E = c.num_experts;
    m.world = c.ep_world_size > 0 ? c.ep_world_size : 1; m.Etot = m.E * m.world; m.eps = eps;
    m.x = x; m.xn = pl.xn; m.rl = pl.rl;
    m.gidx = pl.gate_idx + (size_t)layer * S; m.gval = pl.gate_val + (size_t)layer * S;
    m.gv = c.keep_expert_output ? nullptr : m.gval;
    m.lens = lens; m.live_len = live_len; m.live_rpb = live_rpb; m.pdev = pdev;
    m.eall = pl.eall + (size_t)layer * m.E; m.ld_eall = c.num_blocks * m.E; m.layer = layer;
    m.xb_out = a16 ? xb : nullptr; m.xstats_out = dma ? xstats : nullptr;
    m.ws = (char*)pl.moe_ws + (c.debug_taps ? (size_t)layer * pl.moe_ws_bytes : 0);
    m.mw = carve_moe_workspace(m.ws, S, m.E, D, F);
    const MoeRoute r = choose_moe_route(c, S, w, pl);
    add_moe_router(sb, m, r, pl);
    if (r.ep) {
      add_moe_ep(sb, m, r, pl);
    } else {   // "moe_local.*": index + grouped expert FFN + combine with all experts local
      if (r.gate == GateForm::GateIndex) add_moe_gate_index(sb, m, m.mw.mapping, m.mw.acc, m.mw.pos);
      if (r.gate == GateForm::Top1Index) add_moe_top1(sb, m);
      if (r.gate == GateForm::Top1Index || r.gate == GateForm::RouterTail) add_moe_local_index(sb, m);
      const ExpertFfnPlan f = plan_expert_ffn(expert_weights(c, w), S, m.E, D, F, r.norm_in_expert() ? EXPERT_NORM_IN_KERNEL : 0);
      add_moe_local_expert(sb, m, r, f, pl);
      add_moe_local_combine(sb, m, r, f, pl);
    }
    const std::string b = pfx.substr(0, pfx.size() - 1);
    sb.bd.buffers[b + ".gate_idx"] = Buf{m.gidx, (size_t)S * 4};
    sb.bd.buffers[b + ".gate_value"] = Buf{m.gval, (size_t)S * 4};
    sb.bd.buffers[b + ".mapping"] = Buf{m.mw.mapping, (size_t)S * 4};
    sb.bd.buffers[b + ".acc_histogram"] = Buf{m.mw.acc, (size_t)(m.E + 1) * 4};
  }
  if (c.debug_taps) {
    float* tap = pl.taps + (size_t)tap_index * S * D;
    add_stage(sb, pfx + "tap", 0, [=](hipStream_t s) {
      M3_CHECK_HIP(hipMemcpyAsync(tap, x, (size_t)S * D * sizeof(float), hipMemcpyDeviceToDevice, s));
      return 0;
    });
    sb.bd.buffers[pfx.substr(0, pfx.size() - 1) + ".out"] = Buf{tap, (size_t)S * D * 4};
  }
}

extern "C" {

int m3_engine_output_frames(int T) { return T >= 7 ? sub_len(T) : 0; }

m3_engine* m3_engine_create(const m3_engine_config* config, const m3_weight_entry* table, int n_entries) {
  if (!config || !table || n_entries <= 0) {
    set_error("engine_create: null config / weight table");
    return nullptr;
  }
  m3_engine* e = new m3_engine;
  e->cfg = *config;
  const m3_engine_config& c = e->cfg;
  auto fail = [&](const char* msg) -> m3_engine* {
    if (msg) set_error("%s", msg);
    delete e;
    return nullptr;
  };
  if (c.attention_dim % c.attention_heads || c.embed_dim % c.embed_heads) return fail("engine_create: dim % heads != 0");
  if (c.attention_dim % 16 || c.embed_dim % 16 || c.hidden_units % 64 || c.embed_linear_units % 16)
    return fail("engine_create: dims must be multiples of 16 (hidden_units of 64)");
  if (c.embed_dim != c.attention_dim) return fail("engine_create: embed_dim != attention_dim is not supported");
  if (c.weight_dtype != M3_F32 && c.weight_dtype != M3_BF16 && c.weight_dtype != M3_FP8 && c.weight_dtype != M3_MXFP4)
    return fail("engine_create: weight_dtype must be f32, bf16, fp8 or mxfp4");
  if (c.weight_dtype == M3_MXFP4 && (c.attention_dim % 128 || c.hidden_units % 64))
    return fail("engine_create: mxfp4 experts need an attention_dim that is a multiple of 128 and hidden_units that are a multiple of 64");
  if (c.weight_dtype == M3_MXFP4 && (c.ep_world_size > 1 || c.ep_stages > 0))
    return fail("engine_create: expert parallelism (ep_world_size > 1, ep_stages) is not supported with mxfp4 expert weights");
  if (c.weight_dtype == M3_FP8 && (c.attention_dim % 64 || c.hidden_units % 64))
    return fail("engine_create: fp8 experts need attention_dim and hidden_units that are multiples of 64");
  if (c.fp8_activations && c.weight_dtype != M3_FP8) return fail("engine_create: fp8_activations needs weight_dtype fp8");
  if (c.ep_stages > 0 && c.fuse_route) return fail("engine_create: ep_stages needs the staged route (fuse_route = 0)");
  if (c.ep_world_size > 1 && (c.ep_rank < 0 || c.ep_rank >= c.ep_world_size)) return fail("engine_create: ep_rank outside [0, ep_world_size)");
  if (c.weight_dtype != M3_F32) {
    if (c.fuse_route) return fail("engine_create: fuse_route is fp32-only");
    if (c.attention_dim % 32 || c.hidden_units % 64 || c.embed_linear_units % 32)
      return fail("engine_create: bf16 weights need dims that are multiples of 32");
  }
  e->names.reserve(n_entries);
  for (int i = 0; i < n_entries; ++i) {
    if (!table[i].name || !table[i].data) return fail("engine_create: null weight entry");
    e->names.emplace_back(table[i].name);
    m3_weight_entry w = table[i];
    w.name = nullptr;
    e->table[e->names.back()] = w;
  }
  const int D = c.attention_dim, De = c.embed_dim, K = c.cnn_module_kernel;
  if (!load_sub(e, "embed.subsampling.", De, c.input_dim, &e->sub_e) || !load_sub(e, "subsampling.", D, c.input_dim, &e->sub_m))
    return fail(nullptr);
  if (!load_norm(e, "embed.after_norm.", De, &e->e_after) ||
      !load_lin_ln(e, "out_linear.", c.output_dim, D, false, &e->out_linear))
    return fail(nullptr);
  {   // optional front / back end tensors
    auto m = e->table.find("cmvn.mean"), v = e->table.find("cmvn.istd"), ob = e->table.find("output_bias");
    if ((m == e->table.end()) != (v == e->table.end())) return fail("engine_create: cmvn.mean and cmvn.istd go together");
    if (m != e->table.end()) {
      if (m->second.numel != c.input_dim || v->second.numel != c.input_dim) return fail("engine_create: cmvn vectors must have input_dim entries");
      e->cmvn_mean = (const float*)m->second.data;
      e->cmvn_istd = (const float*)v->second.data;
    }
    if (ob != e->table.end()) {
      if (ob->second.numel != c.output_dim) return fail("engine_create: output_bias must have output_dim entries");
      e->output_bias = (const float*)ob->second.data;
    }
  }
  {
    auto it = e->table.find("pe");
    if (it == e->table.end() || it->second.numel % D) return fail("engine_create: positional table 'pe' missing");
    e->pe = (const float*)it->second.data;
    e->pe_rows = it->second.numel / D;
  }
  if (!lookup(e, "pos_all.weight", (int64_t)(c.embed_blocks + c.num_blocks) * D * D, &e->pos_all,
              c.weight_dtype == M3_F32 ? M3_F32 : M3_BF16))
    return fail(nullptr);
  if (c.fuse_route && !lookup(e, "router_e_all.weight", (int64_t)c.num_blocks * c.num_experts * De, &e->router_e_all))
    return fail(nullptr);
  e->eblocks.resize(c.embed_blocks);
  for (int i = 0; i < c.embed_blocks; ++i)
    if (!load_block(e, "embed.blocks." + std::to_string(i) + ".", De, c.embed_linear_units, K, c.embed_cnn_layer_norm,
                    false, De, &e->eblocks[i], c.embed_causal > 0))
      return fail(nullptr);
  e->mblocks.resize(c.num_blocks);
  for (int i = 0; i < c.num_blocks; ++i)
    if (!load_block(e, "blocks." + std::to_string(i) + ".", D, c.hidden_units, K, c.cnn_layer_norm, true, De,
                    &e->mblocks[i], c.causal > 0))
      return fail(nullptr);
  return e;
}

void m3_engine_destroy(m3_engine* engine) {
  if (!engine) return;
  if (engine->ev_fork) (void)hipEventDestroy(engine->ev_fork);
  if (engine->ev_join) (void)hipEventDestroy(engine->ev_join);
  if (engine->side) (void)hipStreamDestroy(engine->side);
  if (engine->cur.graph_exec) (void)hipGraphExecDestroy(engine->cur.graph_exec);
  for (auto& b : engine->parked)
    if (b.graph_exec) (void)hipGraphExecDestroy(b.graph_exec);
  delete engine;
}

size_t m3_engine_workspace_size(const m3_engine* engine, int B, int T) {
  if (!engine || B <= 0 || T < 7) return 0;
  return make_plan(*engine, nullptr, B, T, engine->ep_capacity).bytes;
}

// once, outside graph capture (idempotent): the dynamic-LDS opt-ins and the like of every kernel family a stage list can hold
static int init_engine_kernels() {
  int (*const inits[])() = {init_expert_ffn_kernels, init_expert_ffn_bf16_kernels, init_expert_ffn_w8_kernels, init_gemm_bf16_tiled_kernels,
                            init_expert_ffn_f32_tiled_kernels, init_expert_ffn_fused_fp8_kernels, init_gemm_f32_tiled_kernels,
                            init_gemm_bf16_dma_kernels, init_expert_gemm_g256_kernels, init_moe_router_kernels,
                            init_relpos_attention_bf16_kernels, init_gemm_f32_splitk_kernels, init_expert_ffn_w4_kernels};
  for (auto init : inits)
    if (int rc = init()) return rc;
  return 0;
}

// The binding of key k, built into bd (a fresh Bound).  Every step that can fail comes before the first one that touches the
// engine (registering a new folded positional table), so a build that fails leaves the engine exactly as it was.
static int build_binding(m3_engine* e, const BindKey& k, m3_engine::Bound& bd) {
  M3_REQUIRE(k.feat && k.feat_len && k.logits && k.ws, "engine_prepare: null argument");
  const int B = k.B, T = k.T;
  M3_REQUIRE(B > 0 && T >= 7, "engine_prepare: need B > 0 and T >= 7 frames (got B=%d T=%d)", B, T);
  const m3_engine_config& c = e->cfg;
  const int Tp = sub_len(T);
  M3_REQUIRE(Tp < e->pe_rows, "engine_prepare: T'=%d exceeds the positional table (%lld rows)", Tp,
             (long long)e->pe_rows);  // rel_positional_encoding_plugin.cpp:139-142
  if (int rc = init_engine_kernels()) return rc;
  const bool streaming = k.sstate != nullptr;
  StageBuilder sb{*e, make_plan(*e, k.ws, B, T, k.ep_cap), bd,
                  streaming ? carve_stream_state(c, k.sstate, B, k.s_hist) : StreamState()};
  Plan& pl = sb.pl;
  M3_REQUIRE(k.ws_bytes >= pl.bytes, "engine_prepare: workspace %zu bytes < required %zu", k.ws_bytes, pl.bytes);
  const int32_t* feat_len = k.feat_len; float* logits = k.logits;
  bd.key = k; bd.Tp = Tp; bd.S = B * Tp;
  sb.splitk_ws = pl.splitk; sb.splitk_bytes = pl.splitk_bytes;
  {
    // bf16 activation operands need every GEMM that reads or rewrites them on the LDS-tiled kernel: the narrowest ones
    // are the D x D projections (the expert-parallel driver's combine op writes the bf16 copy too: m3_moe_combine_bf16)
    GemmParams t;
    t.M = B * Tp; t.N = c.attention_dim; t.K = c.attention_dim; t.w_bf16 = 1;
    bd.a16 = c.weight_dtype != M3_F32 && c.bf16_activations >= 0 && !c.debug_taps && c.embed_dim == c.attention_dim &&
             (c.embed_linear_units % 128) == 0 && (c.hidden_units % 128) == 0 && plan_gemm(t, 0).kernel == GemmKernel::TiledBf16;
  }
  {
    GemmParams t;     // the narrowest block GEMM as the LDS-DMA kernel would see it
    t.M = B * Tp; t.N = c.attention_dim; t.K = c.attention_dim; t.lda = c.attention_dim; t.w_bf16 = 1; t.a_bf16 = 1;
    bd.dma = bd.a16 && c.attention_dim == 128 * kXbStatParts && plan_gemm(t, 0).kernel == GemmKernel::DmaBf16;
  }
  bd.packed = use_packed_rows(c, B);
  if (streaming) {   // a chunk is a few rows per utterance: padded layout, fp32 activations (the 16-bit modes keep their bf16 weights)
    bd.a16 = bd.dma = bd.packed = false;   // (the plan's packed-row buffers stay carved, unused)
  }
  const int S = bd.S, D = c.attention_dim, De = c.embed_dim;

  if (pl.ep_overflow != nullptr) {   // bounded expert-parallel wire: the overflow report of this forward starts at 0
    int32_t* ovf = pl.ep_overflow;
    add_stage(sb, "ep.reset", 0, [=](hipStream_t s) {
      M3_CHECK_HIP(hipMemsetAsync(ovf, 0, sizeof(int32_t), s));
      return 0;
    });
    bd.buffers["ep.overflow"] = Buf{ovf, sizeof(int32_t)};
  }
  // valid lengths after the two stride-2 convs (MaskConv2dSample x2, subsampling.py:119-137)
  {
    // No launch of their own: the packed layout's row plan forms them on its way; otherwise the forward's first kernel (the
    // embed subsampler's conv1) does.  Exceptions that keep the separate "lens" stage: a forked capture (the main branch reads
    // the lengths while the embed branch, whose conv1 would write them, runs beside it) and a positional projection that is
    // not folded (its GEMM would sit in front of conv1 -- harmless, but the stage order of round 1 is kept for it).
    int32_t* lens = pl.lens;
    if (bd.packed) {   // row plan of the packed layout: first row of every utterance, packed -> padded row map
      int32_t* row0 = pl.row0; int32_t* pad_of = pl.pad_of;
      add_stage(sb, "pack_plan", 1, [=](hipStream_t s) { return launch_pack_plan(lens, B, Tp, row0, pad_of, s, feat_len); },
                stage_info("pack_plan_kernel", 1, 12.0 * B + 4.0 * B * Tp, 0.0, false));
    } else if (pl.fork || (!c.fold_pos_proj && !streaming)) {
      add_stage(sb, "lens", 1, [=](hipStream_t s) { return launch_subsample_lens(feat_len, B, lens, s); },
                stage_info("subsample_lens_kernel", 1, 8.0 * B, 0.0, false));
    } else {
      sb.lens_in_conv1 = true;
    }
  }
  // ---- p = linear_pos(pe[:T']) for all blocks at once (attention.py:345; input-independent, so with
  //      fold_pos_proj it is computed once per bound shape instead of once per forward) ----
  {
    const int nb = c.num_blocks + c.embed_blocks;
    GemmParams pp;
    // (streaming: keys carry their ABSOLUTE position, rel_positional_encoding_kernel.cu:108-111 pe[offset : offset + T]: one
    //  table over the s_maxf positions a stream can reach, always folded)
    const int Tpos = streaming ? k.s_maxf : Tp;
    pp.A = e->pe; pp.lda = D; pp.W = e->pos_all; pp.Y = pl.pbuf; pp.ldy = nb * D; pp.M = Tpos; pp.N = nb * D; pp.K = D;
    if (c.fold_pos_proj || streaming) {
      auto known = e->pfold_by_tp.find(Tpos);
      std::shared_ptr<float> pf = known != e->pfold_by_tp.end() ? known->second.lock() : nullptr;
      if (!pf) {
        float* dev = nullptr;
        M3_CHECK_HIP(hipMalloc((void**)&dev, (size_t)Tpos * nb * D * sizeof(float)));
        pf = std::shared_ptr<float>(dev, [](float* q) { (void)hipFree(q); });
        pp.Y = dev;
        pp.w_bf16 = c.weight_dtype != M3_F32;
        if (int rc = launch_gemm(gemm_launch(pp, nullptr, 0), nullptr)) return rc;
        M3_CHECK_HIP(hipStreamSynchronize(nullptr));
        // (nothing below can fail: from here on the engine may change)
        for (auto it = e->pfold_by_tp.begin(); it != e->pfold_by_tp.end();)      // tables no binding holds any more
          it = it->second.expired() ? e->pfold_by_tp.erase(it) : std::next(it);
        e->pfold_by_tp[Tpos] = pf;
      }
      bd.pfold = pf;
      pl.pbuf = pf.get();
    } else {
      add_gemm(sb, "pos_all", pp);
    }
  }
  // ---- embed encoder (conformer_embed_domain_acc.py:149-181) ----
  const Plan ple = embed_view(pl);
  const int embed_start = (int)bd.stages.size();    // the embed chain starts here ...
  sb.splitk_ws = ple.splitk;
  build_subsample(sb, "embed.subsample.", e->sub_e, De, ple, ple.x);
  for (int i = 0; i < c.embed_blocks; ++i) {
    if (i + 1 == c.embed_blocks) {   // after_norm joins the last block's norm_final launch
      sb.tail_ln_g = e->e_after.g; sb.tail_ln_b = e->e_after.b; sb.tail_ln_eps = 1e-12f; sb.tail_ln_out = pl.emb;
    }
    build_block(sb, "embed.blocks." + std::to_string(i) + ".", e->eblocks[i], De, c.embed_linear_units, c.embed_heads,
                c.cnn_module_kernel, c.embed_cnn_layer_norm, false, i, i, ple, c.embed_causal > 0);
  }
  sb.splitk_ws = pl.splitk;
  if (c.embed_blocks == 0) {
    float* x = ple.x; float* emb = pl.emb;
    const float* g = e->e_after.g; const float* b = e->e_after.b;
    add_stage(sb, "embed.after_norm", 1, [=](hipStream_t s) { return launch_layernorm(x, g, b, 1e-12f, emb, S, De, s); },
              stage_info("layernorm_kernel", 1, 8.0 * S * De, 8.0 * S * De));
  }
  // embed half of every layer's router product in one GEMM: emb does not change across the main blocks
  if (choose_moe_route(c, S, e->mblocks.empty() ? BlockW() : e->mblocks[0], pl).needs_e_all) {
    GemmParams g;
    g.A = pl.emb; g.lda = De; g.W = e->router_e_all; g.Y = pl.eall; g.ldy = c.num_blocks * c.num_experts;
    g.M = S; g.N = c.num_blocks * c.num_experts; g.K = De;
    add_gemm(sb, "router_e_all", g, true);
    bd.stages.back().reads_embed = true;
  }
  // ... or, staged fp32 router of short inputs, as the accumulators every layer's router GEMM starts from: the same bits as the
  // whole-K GEMM, half the operand pull on each layer's critical path (router_prefix_layer_floats)
  if (pl.rprefix != nullptr) {
    GemmParams g = router_concat_gemm(c, S, pl.emb, pl.x);
    g.W = e->mblocks[0].router.w; g.Y = pl.rl; g.ln_gamma = e->mblocks[0].n_ff.g; g.ln_beta = e->mblocks[0].n_ff.b; g.acc_init = pl.rprefix;
    if (bd.packed) g.m_dev = pl.row0 + B;
    const GemmPlan plan = plan_gemm(g, 0);
    M3_REQUIRE(plan.launches == 1 && router_prefix_floats(plan) == pl.rprefix_layer, "engine_prepare: router prefix: %s", plan.reason);
    std::vector<const float*> wt(kRouterPrefixMaxLayers, nullptr);
    for (int i = 0; i < c.num_blocks; ++i) wt[i] = e->mblocks[i].router.w;
    float* prefix = pl.rprefix; const int L = c.num_blocks;
    const double Etot = g.N;
    add_stage(sb, "router_e_prefix", 1, [plan, g, wt, prefix, L](hipStream_t s) { return launch_router_embed_prefix(plan, g, wt.data(), 0, L, prefix, s); },
              stage_info("router_embed_prefix_kernel", 1, 4.0 * De * (L * Etot + S) + 4.0 * L * pl.rprefix_layer, 2.0 * S * Etot * De * L));
    bd.stages.back().reads_embed = bd.stages.back().router_prefix = true;
  }
  // ---- main MoE encoder (conformer_fmoe_localComm_catEmbed_domain_acc_hier.py:198-234) ----
  const int main_start = (int)bd.stages.size();     // ... and the main encoder here
  build_subsample(sb, "subsample.", e->sub_m, D, pl, pl.x);
  for (int i = 0; i < c.num_blocks; ++i)
    build_block(sb, "blocks." + std::to_string(i) + ".", e->mblocks[i], D, c.hidden_units, c.attention_heads,
                c.cnn_module_kernel, c.cnn_layer_norm, true, i, c.embed_blocks + i, pl, c.causal > 0);
  {
    GemmParams g;
    g.A = pl.x; g.lda = D; g.W = e->out_linear.w; g.bias = e->out_linear.b; g.Y = logits; g.ldy = c.output_dim;
    g.M = S; g.N = c.output_dim; g.K = D;
    g.ln_wsum = e->out_linear.wsum; g.ln_eps = 1e-12f;       // after_norm is folded into out_linear
    if (bd.a16) { g.A = (const float*)pl.xb; g.a_bf16 = 1; }
    if (bd.dma) { g.ln_stats = pl.xstats; g.ln_stat_parts = kXbStatParts; }
    float* lout = logits;
    if (bd.packed) {   // packed rows -> packed logits; the (B, T', V) output is filled from them at the end
      lout = pl.lpk;
      g.Y = lout;
      g.m_dev = pl.row0 + B;
    }
    add_gemm(sb, "logits", g);
    const float* ob = e->output_bias;
    const int V = c.output_dim;
    if (c.log_softmax_out) {
      add_stage(sb, "log_softmax", 1, [=](hipStream_t s) { return launch_log_softmax_bias(lout, ob, lout, (size_t)S, V, s); },
                stage_info("log_softmax_bias_kernel", 1, 8.0 * S * V, 4.0 * S * V));
    }   // without log-softmax a prior is folded into out_linear's bias when the plan is packed (plan.py)
    if (bd.packed) {
      const int32_t* row0 = pl.row0;
      add_stage(sb, "unpack", 1, [=](hipStream_t s) { return launch_unpack_rows(lout, row0, B, Tp, V, logits, s); },
                stage_info("unpack_rows_kernel", 1, 8.0 * S * V, 0.0, false));
    }
  }
  // the main encoder first needs the embedding at blocks.0's router: the forked capture joins its two branches there, horizontal
  // fusion interleaves the two chains up to there
  const int join = embed_join(bd.stages, main_start);
  if (pl.fork && join >= 0 && c.num_blocks >= 1) {
    bd.fork_first = embed_start; bd.fork_mid = main_start; bd.join_at = join;
  }
  if (pl.hfuse && !streaming && join > 0) fuse_independent_pairs(sb, embed_start, main_start, join);
  if (streaming) {   // the chunk counter moves on the device: the same captured graph serves every chunk of the stream
    const StreamState& st = sb.st;
    int32_t* step = st.step;
    if (k.s_slots) {   // one counter per utterance slot; a slot moves only if it was live in this chunk
      int32_t *pos = st.slot_pos, *status = st.slot_status, *frames = st.slot_frames;
      const int32_t* lens = pl.lens; const int max_chunks = k.s_maxf / Tp;
      add_stage(sb, "stream.advance", 1, [=](hipStream_t s) { return launch_advance_slots(pos, status, frames, lens, B, Tp, max_chunks, s); },
                stage_info("advance_slots_kernel", 1, 20.0 * B, 0.0, false));
    } else
    add_stage(sb, "stream.advance", 1, [=](hipStream_t s) { return launch_advance_counter(step, 1, s); },
              stage_info("advance_counter_kernel", 1, 8.0, 0.0, false));
  }
  for (int i = 0; i < (int)bd.stages.size(); ++i)
    if (bd.stages[i].router_prefix) bd.prefix_stage = i;   // (its index after fuse_independent_pairs has reordered the list)
  bd.buffers["x"] = Buf{pl.x, (size_t)S * D * 4};
  bd.buffers["dw"] = Buf{pl.dw, (size_t)S * D * 4};   // the main encoder's depthwise conv + LayerNorm + SiLU output (last block run)
  if (!bd.xn_skipped) bd.buffers["xn"] = Buf{pl.xn, (size_t)S * D * 4};
  if (pl.xq != nullptr) {
    bd.buffers["xq"] = Buf{pl.xq, (size_t)S * D};
    bd.buffers["xq_scale"] = Buf{pl.xq_scale, (size_t)S * 4};
  }
  bd.buffers["embed"] = Buf{pl.emb, (size_t)S * De * 4};
  if (bd.a16) bd.buffers["xb"] = Buf{pl.xb, (size_t)S * D * 2};
  bd.buffers["lens"] = Buf{pl.lens, (size_t)B * 4};
  if (bd.packed) bd.buffers["row0"] = Buf{pl.row0, (size_t)(B + 1) * 4};
  if (pl.ep_rows) bd.buffers["ep.gate_recv"] = Buf{pl.ep_gate_recv, (size_t)pl.ep_rows * 4};
  bd.buffers["router_logits"] = Buf{pl.rl, (size_t)S * c.num_experts * (c.ep_world_size > 0 ? c.ep_world_size : 1) * 4};

  return 0;
}

// ---- shape cache: the current binding plus up to cfg.shape_cache parked ones, least recently used evicted first ----
static int find_parked(const m3_engine* e, const BindKey& k) {
  for (size_t i = 0; i < e->parked.size(); ++i)
    if (e->parked[i].matches(k)) return (int)i;
  return -1;
}

static int shape_cache_capacity(const m3_engine* e) { return e->cfg.shape_cache > 0 ? e->cfg.shape_cache : (e->cfg.shape_cache < 0 ? 0 : 7); }

// the parked binding that parking one more evicts: the least recently used one of a full cache (-1: there is room)
static int park_victim(const m3_engine* e) {
  if (e->parked.empty() || (int)e->parked.size() < shape_cache_capacity(e)) return -1;
  size_t lru = 0;
  for (size_t i = 1; i < e->parked.size(); ++i)
    if (e->parked[i].last_use < e->parked[lru].last_use) lru = i;
  return (int)lru;
}

// the current binding moves to the parked ones (cache capacity 0: it is dropped) and leaves e->cur empty
static void park_current(m3_engine* e) {
  if (e->cur.stages.empty()) return;
  if (shape_cache_capacity(e) > 0) {
    const int victim = park_victim(e);
    if (victim >= 0) {
      if (e->parked[victim].graph_exec) (void)hipGraphExecDestroy(e->parked[victim].graph_exec);
      e->parked.erase(e->parked.begin() + victim);
    }
    e->parked.push_back(std::move(e->cur));
  } else if (e->cur.graph_exec) {
    (void)hipGraphExecDestroy(e->cur.graph_exec);
  }
  e->cur = m3_engine::Bound();
}

// Makes the binding of key k the current one: it is the current one already, or a parked one is revived, or it is built.
// Build, then commit: a new binding is built aside and the engine changes only once it is complete.  (The current binding is
// parked BEFORE the parked ones are searched, so a wanted binding that this parking evicts is built anew.)
static int bind(m3_engine* e, const BindKey& k) {
  if (!e->cur.matches(k)) {
    int hit = find_parked(e, k);
    if (hit >= 0 && !e->cur.stages.empty() && hit == park_victim(e)) hit = -1;
    m3_engine::Bound fresh;
    if (hit < 0)
      if (int rc = build_binding(e, k, fresh)) return rc;
    park_current(e);
    if (hit >= 0) {
      hit = find_parked(e, k);
      fresh = std::move(e->parked[hit]);
      e->parked.erase(e->parked.begin() + hit);
    }
    e->cur = std::move(fresh);
  }
  e->cur.last_use = ++e->use_clock;
  return 0;
}

// the key of a whole-utterance binding (m3_engine_prepare / m3_engine_forward)
static BindKey forward_key(const m3_engine* e, const float* feat, const int32_t* feat_len, int B, int T, float* logits,
                           void* workspace, size_t workspace_bytes) {
  BindKey k;
  k.B = B; k.T = T; k.feat = feat; k.feat_len = feat_len; k.logits = logits; k.ws = workspace; k.ws_bytes = workspace_bytes;
  k.ep_cap = e->ep_capacity;
  return k;
}

int m3_engine_prepare(m3_engine* e, const float* feat, const int32_t* feat_len, int B, int T, float* logits,
                      void* workspace, size_t workspace_bytes) {
  M3_REQUIRE(e != nullptr, "engine_prepare: null argument");
  if (int rc = bind(e, forward_key(e, feat, feat_len, B, T, logits, workspace, workspace_bytes))) return rc;
  return (int)e->cur.stages.size();
}

int m3_engine_set_ep_capacity(m3_engine* engine, int rows_per_chunk) {
  M3_REQUIRE(engine != nullptr && rows_per_chunk >= 0, "engine_set_ep_capacity: bad argument");
  engine->ep_capacity = rows_per_chunk;
  return 0;
}

int m3_engine_num_stages(const m3_engine* engine) { return engine ? (int)engine->cur.stages.size() : 0; }
const char* m3_engine_stage_name(const m3_engine* engine, int index) {
  if (!engine || index < 0 || index >= (int)engine->cur.stages.size()) return nullptr;
  return engine->cur.stages[index].name.c_str();
}
int m3_engine_num_captures(const m3_engine* engine) { return engine ? engine->n_captures : 0; }
int m3_engine_stage_info(const m3_engine* engine, int index, m3_stage_info* info) {
  M3_REQUIRE(engine && info, "engine_stage_info: null argument");
  M3_REQUIRE(index >= 0 && index < (int)engine->cur.stages.size(), "engine_stage_info: no stage %d", index);
  *info = engine->cur.stages[index].info;
  return 0;
}
int m3_engine_num_kernels(const m3_engine* engine) { return engine ? engine->cur.n_kernels : 0; }

// Stages [first, last) of the current binding.  A caller that runs stages piecewise may change a router's weights between two
// calls (the calibration does: it runs up to a layer's router, edits that router, runs the router stage again), and the routers'
// accumulator prefix was formed from the weights as they stood when "router_e_prefix" ran.  So a router stage that is reached
// without the prefix stage in front of it IN THIS CALL first recomputes its own layer's slice, on the same stream: the stage
// then computes what the whole-K GEMM would, whatever happened between the calls.  `whole`: the ranges are the pieces of one
// forward (forked capture), the prefix stage has run in an earlier piece.
static int run_stage(const Stage& st, hipStream_t stream) {
  if (auto* g = std::get_if<GemmLaunch>(&st.launch)) return launch_gemm(*g, stream);
  if (auto* c = std::get_if<Conv1Args>(&st.launch)) return launch_conv1_relu(*c, stream);
  if (auto* d = std::get_if<DwArgs>(&st.launch)) return launch_dwconv_ln_silu(*d, stream);
  if (auto* t = std::get_if<AttArgs>(&st.launch)) return launch_relpos_attention(*t, stream);
  return st.run(stream);
}
static int run_stage_range(m3_engine* engine, int first_stage, int last_stage, hipStream_t stream, bool whole) {
  const int ps = engine->cur.prefix_stage;
  for (int i = first_stage; i < last_stage; ++i) {
    const Stage& st = engine->cur.stages[i];
    if (st.refresh_prefix && !whole && !(ps >= first_stage && ps < i))
      if (int rc = st.refresh_prefix(stream)) return rc;
    if (int rc = run_stage(st, stream)) return rc;
  }
  return 0;
}

int m3_engine_run(m3_engine* engine, int first_stage, int last_stage, m3_stream stream) {
  M3_REQUIRE(engine && !engine->cur.stages.empty(), "engine_run: engine not prepared");
  M3_REQUIRE(first_stage >= 0 && last_stage <= (int)engine->cur.stages.size() && first_stage <= last_stage,
             "engine_run: bad stage range [%d,%d)", first_stage, last_stage);
  return run_stage_range(engine, first_stage, last_stage, (hipStream_t)stream, false);
}

int m3_engine_buffer(const m3_engine* engine, const char* name, void** ptr, size_t* bytes) {
  M3_REQUIRE(engine && name && ptr && bytes, "engine_buffer: null argument");
  auto it = engine->cur.buffers.find(name);
  M3_REQUIRE(it != engine->cur.buffers.end(), "engine_buffer: no buffer named '%s' for the bound shape", name);
  *ptr = it->second.ptr;
  *bytes = it->second.bytes;
  return 0;
}

// Captures the current binding's stage list on `stream` and instantiates the graph.  A binding built for fork_embed runs the
// embed encoder as a side branch.  `who` names the entry point in the messages.
static int capture_graph(m3_engine* e, hipStream_t stream, const char* who) {
  m3_engine::Bound& b = e->cur;
  M3_REQUIRE(stream != nullptr, "%s: graph capture needs a non-default stream", who);
  if (b.graph_exec) {
    (void)hipGraphExecDestroy(b.graph_exec);
    b.graph_exec = nullptr;
  }
  hipGraph_t graph = nullptr;
  const int n_st = (int)b.stages.size();
  const bool fork = b.fork_first >= 0 && b.fork_mid > b.fork_first && b.join_at > b.fork_mid;
  if (fork && e->side == nullptr) {
    M3_CHECK_HIP(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
    M3_CHECK_HIP(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    M3_CHECK_HIP(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
  }
  M3_CHECK_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
  int rc = 0;
  if (!fork) {
    rc = run_stage_range(e, 0, n_st, stream, true);
  } else {
    // two branches between "lens" and blocks.0's router: the embed encoder on the side stream (it joins the capture through
    // the fork event), the main subsampler + block 0 up to its router on the capture stream
    hipError_t he = hipSuccess;
    rc = run_stage_range(e, 0, b.fork_first, stream, true);
    if (!rc && (he = hipEventRecord(e->ev_fork, stream)) != hipSuccess) rc = -1;
    if (!rc && (he = hipStreamWaitEvent(e->side, e->ev_fork, 0)) != hipSuccess) rc = -1;
    if (!rc) rc = run_stage_range(e, b.fork_first, b.fork_mid, e->side, true);
    if (!rc) rc = run_stage_range(e, b.fork_mid, b.join_at, stream, true);
    if (!rc && (he = hipEventRecord(e->ev_join, e->side)) != hipSuccess) rc = -1;
    if (!rc && (he = hipStreamWaitEvent(stream, e->ev_join, 0)) != hipSuccess) rc = -1;
    if (!rc) rc = run_stage_range(e, b.join_at, n_st, stream, true);
    if (he != hipSuccess) set_error("%s: forked capture failed: %s", who, hipGetErrorString(he));
  }
  hipError_t ce = hipStreamEndCapture(stream, &graph);
  if (rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  M3_CHECK_HIP(ce);
  M3_CHECK_HIP(hipGraphInstantiate(&b.graph_exec, graph, nullptr, nullptr, 0));
  M3_CHECK_HIP(hipGraphDestroy(graph));
  b.graph_valid = true;
  ++e->n_captures;
  return 0;
}

// the current binding once: stage by stage, or as one replay of its graph (captured on first use)
static int run_current(m3_engine* e, int use_graph, m3_stream stream_, const char* who) {
  if (!use_graph) return m3_engine_run(e, 0, (int)e->cur.stages.size(), stream_);
  hipStream_t stream = (hipStream_t)stream_;
  if (!e->cur.graph_valid)
    if (int rc = capture_graph(e, stream, who)) return rc;
  M3_CHECK_HIP(hipGraphLaunch(e->cur.graph_exec, stream));
  return 0;
}

int m3_engine_forward(m3_engine* e, const float* feat, const int32_t* feat_len, int B, int T, float* logits,
                      void* workspace, size_t workspace_bytes, int use_graph, m3_stream stream_) {
  M3_REQUIRE(e != nullptr, "engine_forward: null engine");
  if (int rc = bind(e, forward_key(e, feat, feat_len, B, T, logits, workspace, workspace_bytes))) return rc;
  M3_REQUIRE(e->cfg.ep_world_size <= 1, "engine_forward: an expert-parallel engine (ep_world_size = %d) is run stage-wise, with the "
             "all-to-all between its moe_ep.* stages (m3asr/ep.py)", (int)e->cfg.ep_world_size);
  return run_current(e, use_graph, stream_, "engine_forward");
}


// ------------------------------------------------------------------------------------------------------------------------
// Chunk-by-chunk (streaming) execution: decoding-chunk semantics of trainer_3m_fix/model/encoder.py:100-140
// (decoding_chunk_size / num_decoding_left_chunks -> add_optional_chunk_mask) with the caches the reference's streaming plugins
// were written for (cat_split_cache_kernel.cu:30-107, att_stream_softmax_kernel.cu:136-191,
// rel_positional_encoding_kernel.cu:108-123).  Contract: with static_chunk_size = c, causal conv modules in both encoders and
// the same weights, the logits of chunk n equal rows [n c, (n + 1) c) of the full-utterance forward (m3_engine_forward) up to
// fp32 rounding of the GEMMs (their kernels are chosen by row count); the attention core and the conv are bit-exact.
static int stream_check(const m3_engine* e, const m3_stream_desc* d) {
  M3_REQUIRE(e != nullptr && d != nullptr, "engine stream: null argument");
  const m3_engine_config& c = e->cfg;
  M3_REQUIRE(c.static_chunk_size > 0, "engine stream: the engine was built without static_chunk_size (the chunk length in output frames)");
  M3_REQUIRE(c.causal > 0 && c.embed_causal > 0, "engine stream: both encoders need causal conv modules (a symmetric depthwise conv "
             "looks %d frames into the future)", (int)(c.cnn_module_kernel - 1) / 2);
  M3_REQUIRE(c.ep_world_size <= 1 && c.ep_stages <= 0 && c.fork_embed <= 0, "engine stream: expert-parallel stages / forked capture are not available chunk by chunk");
  M3_REQUIRE(d->B > 0 && d->max_frames >= c.static_chunk_size && d->max_frames < e->pe_rows,
             "engine stream: need B > 0 and chunk <= max_frames < %lld positions (got B=%d max_frames=%d)", (long long)e->pe_rows, d->B, d->max_frames);
  const int need = c.num_left_chunks < 0 ? d->max_frames : (c.num_left_chunks + 1) * c.static_chunk_size;
  M3_REQUIRE(d->history_frames >= need, "engine stream: history_frames=%d < %d (%s)", d->history_frames, need,
             c.num_left_chunks < 0 ? "all left chunks are visible: the history must hold the whole stream" : "(num_left_chunks + 1) chunks");
  return 0;
}

// stream_check, then "the caller's state is there and large enough": the state carved into *st.  `who` names the entry point
static int stream_state(const m3_engine* e, const m3_stream_desc* d, const void* state, size_t state_bytes, const char* who,
                        StreamState* st) {
  if (int rc = stream_check(e, d)) return rc;
  *st = carve_stream_state(e->cfg, const_cast<void*>(state), d->B, d->history_frames);
  M3_REQUIRE(state != nullptr && state_bytes >= st->bytes, "%s: state %zu bytes < required %zu", who, state_bytes, st->bytes);
  return 0;
}

int m3_engine_chunk_input_frames(const m3_engine* engine) {
  // c output frames need input frames [4 j0, 4 (j0 + c - 1) + 6]: 4 c + 3 of them, advancing by 4 c per chunk (7-frame context of
  // the two stride-2 3x3 convs, subsampling.py:103-145)
  return engine && engine->cfg.static_chunk_size > 0 ? 4 * engine->cfg.static_chunk_size + 3 : 0;
}

size_t m3_engine_stream_state_size(const m3_engine* engine, const m3_stream_desc* desc) {
  if (stream_check(engine, desc)) return 0;
  return carve_stream_state(engine->cfg, nullptr, desc->B, desc->history_frames).bytes;
}

int m3_engine_stream_reset(m3_engine* e, const m3_stream_desc* desc, void* state, size_t state_bytes, m3_stream stream_) {
  StreamState st;
  if (int rc = stream_state(e, desc, state, state_bytes, "engine_stream_reset", &st)) return rc;
  const m3_engine_config& c = e->cfg;
  hipStream_t stream = (hipStream_t)stream_;
  M3_CHECK_HIP(hipMemsetAsync(st.step, 0, 64 * sizeof(int32_t), stream));
  M3_CHECK_HIP(hipMemsetAsync(st.slot_pos, 0, (size_t)3 * desc->B * sizeof(int32_t), stream));
  // the K-1 frames left of frame 0 are what the conv module's zero padding becomes behind pointwise_conv1 + GLU
  const int K = c.cnn_module_kernel, D = c.attention_dim, nb = c.embed_blocks + c.num_blocks;
  for (int i = 0; i < nb; ++i) {
    const BlockW& w = i < c.embed_blocks ? e->eblocks[i] : e->mblocks[i - c.embed_blocks];
    if (int rc = launch_fill_rows(w.left_fill, D, st.conv[i], (size_t)2 * desc->B * (K - 1), stream)) return rc;
  }
  return 0;
}

// bind (or revive) the chunk binding of this (state, buffers, mode) and run it: eagerly, or as one hipGraph replay
static int run_chunk(m3_engine* e, const m3_stream_desc* desc, void* state, const float* feat_chunk, const int32_t* chunk_feat_len,
                     float* logits, void* workspace, size_t workspace_bytes, bool slots, int use_graph, m3_stream stream_) {
  BindKey k = forward_key(e, feat_chunk, chunk_feat_len, desc->B, 4 * e->cfg.static_chunk_size + 3, logits, workspace, workspace_bytes);
  k.sstate = state; k.s_hist = desc->history_frames; k.s_maxf = desc->max_frames; k.s_slots = slots;
  if (int rc = bind(e, k)) return rc;
  return run_current(e, use_graph, stream_, "engine_forward_chunk");
}

int m3_engine_forward_chunk(m3_engine* e, const m3_stream_desc* desc, void* state, size_t state_bytes, const float* feat_chunk,
                            const int32_t* chunk_feat_len, float* logits, void* workspace, size_t workspace_bytes, int chunk_index,
                            int use_graph, m3_stream stream_) {
  StreamState st;
  if (int rc = stream_state(e, desc, state, state_bytes, "engine_forward_chunk", &st)) return rc;
  M3_REQUIRE(chunk_index >= 0 && (long)(chunk_index + 1) * e->cfg.static_chunk_size <= desc->max_frames,
             "engine_forward_chunk: chunk %d ends past max_frames=%d (the stream is longer than the state was sized for)", chunk_index, desc->max_frames);
  return run_chunk(e, desc, state, feat_chunk, chunk_feat_len, logits, workspace, workspace_bytes, false, use_graph, stream_);
}

// ---- slot mode: the B streams of a state start, pause and end independently ------------------------------------------------
// Position is a property of the slot: the attention core, the depthwise conv and stream.advance read utterance b's own chunk
// counter (StreamState::slot_pos), and a slot with no output frame in a chunk (or one that would run past max_frames) is left
// exactly as it was.  Which slots are live is device data (chunk_feat_len), so every chunk is still one replay of one graph.
int m3_engine_forward_chunk_slots(m3_engine* e, const m3_stream_desc* desc, void* state, size_t state_bytes, const float* feat_chunk,
                                  const int32_t* chunk_feat_len, float* logits, void* workspace, size_t workspace_bytes,
                                  int use_graph, m3_stream stream_) {
  StreamState st;
  if (int rc = stream_state(e, desc, state, state_bytes, "engine_forward_chunk_slots", &st)) return rc;
  return run_chunk(e, desc, state, feat_chunk, chunk_feat_len, logits, workspace, workspace_bytes, true, use_graph, stream_);
}

int m3_engine_stream_reset_slots(m3_engine* e, const m3_stream_desc* desc, void* state, size_t state_bytes, const int32_t* slots,
                                 int n, m3_stream stream_) {
  StreamState st;
  if (int rc = stream_state(e, desc, state, state_bytes, "engine_stream_reset_slots", &st)) return rc;
  const m3_engine_config& c = e->cfg;
  M3_REQUIRE(n >= 0 && (n == 0 || slots != nullptr), "engine_stream_reset_slots: bad slot list (n=%d)", n);
  const int nb = c.embed_blocks + c.num_blocks;
  M3_REQUIRE(nb <= kMaxStreamBlocks, "engine_stream_reset_slots: %d blocks > %d", nb, kMaxStreamBlocks);
  SlotResetArgs a;
  a.pos = st.slot_pos; a.status = st.slot_status; a.frames = st.slot_frames; a.slots = slots; a.n = n;
  a.B = desc->B; a.K = c.cnn_module_kernel; a.D = c.attention_dim; a.n_blocks = nb;
  for (int i = 0; i < kMaxStreamBlocks; ++i) { a.conv[i] = nullptr; a.fill[i] = nullptr; }
  for (int i = 0; i < nb; ++i) {
    a.conv[i] = st.conv[i];
    a.fill[i] = (i < c.embed_blocks ? e->eblocks[i] : e->mblocks[i - c.embed_blocks]).left_fill;
  }
  return launch_reset_slots(a, (hipStream_t)stream_);
}

int m3_engine_stream_positions(m3_engine* e, const m3_stream_desc* desc, const void* state, size_t state_bytes, int32_t* frames,
                               m3_stream stream_) {
  StreamState st;
  if (int rc = stream_state(e, desc, state, state_bytes, "engine_stream_positions", &st)) return rc;
  M3_REQUIRE(frames != nullptr, "engine_stream_positions: null pointer");
  return launch_slot_positions(st.slot_status, st.slot_frames, desc->B, frames, (hipStream_t)stream_);
}

}  // extern "C"
