"""The "plan": config + packed fp32 weights -- what replaces TensorRT's serialized engine
(TRTAPI++/python/trt_helper/builder_helper.py:146-167 `build_engine`, infer.py:29-36 deserialize).

``pack_weights`` turns a reference-layout state_dict (the keys of ``Net.state_dict()``, builder.py:131-134)
into the layouts the HIP engine consumes (all build-time host work, done once):
  * LayerNorms that feed exactly one Linear (norm_ff_macaron, norm_mha, norm_conv, dense norm_ff, after_norm)
    are folded into it (`*.ln.weight/bias/wsum`): the GEMM runs on the raw rows and normalises its OUTPUT;
  * q/k/v projections fused into one [3D, D] weight + [3D] bias (one GEMM instead of three Linear layers,
    attention.py:334-343);
  * pointwise Conv1d weights (O, I, 1) viewed as [O, I]; depthwise (C,1,K) -> [K, C] (channel-last rows);
  * subsampling conv1 (C,1,3,3) -> [9, C]; conv2 (O,I,3,3) -> [O,3,3,I] (implicit-GEMM K order);
    the Linear after the convs gets its columns permuted from (c, f) to (f, c) because the engine keeps
    activations channel-last (the reference flattens (B,C,T,F)->(B,T,C*F), subsampling.py:141-142);
  * router_weights [D+De, E] -> transposed [E, D+De]; expert w_2 [E,D,F] -> slice-major [E,F/64,D,64];
  * eval BatchNorm in the conv module (cnn_module_norm='batch_norm') folded into the depthwise conv;
  * the sinusoidal table ``pe`` (positional_encoding.py:40-48) for max_len positions;
  * ``pack_decoder``: the attention decoder of a joint CTC/attention checkpoint (`decoder.*`, fp32 in every mode) for
    m3asr.rescore; its DecoderConfig travels in the header's extra["decoder"], so encoder-only plans are unchanged;
  * in expert-parallel mode only this rank's expert slice [rank*E_loc, (rank+1)*E_loc) is kept
    (load_state_dict_comm, conformer_fmoe_localComm_catEmbed_domain_acc_hier.py:259-273).

File format (``save_plan`` / ``load_plan``): 8-byte magic, u64 header length, JSON header
{config, tensors: {name: [offset, shape]}}, then raw little-endian fp32 data (256-B aligned).
"""
import json
import re
import math
import struct
from collections import OrderedDict

import numpy as np
import torch

from .config import DecoderConfig, EncoderConfig

MAGIC = b"M3ASRPL1"
EXPERT_SLICE = 64    # = m3_moe_expert_slice() of libm3asr_hip.so (checked when an Engine is created)


def positional_table(max_len, d):
    pe = torch.zeros(max_len, d)
    position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def slice_major_w2(t):
    """expert w_2 [E, D, F] -> slice-major [E, F/S, D, S] (S = EXPERT_SLICE): the bytes a workgroup of the grouped expert FFN
    streams in its second GEMM become one contiguous run"""
    E_, D_, F_ = t.shape
    return t.reshape(E_, D_, F_ // EXPERT_SLICE, EXPERT_SLICE).permute(0, 2, 1, 3).contiguous()


def pack_wfrag(t):
    """row-major fp32 [..., N, K] (N, K multiples of 16) -> MFMA-fragment order [..., N/16, K/16, 4 (kq), 16 (col), 4]
    (include/m3asr.h "fragment order"): Wf[nt][s][kq][col][j] = W[16 nt + col][16 s + 4 kq + j], the KB of one (column tile,
    K-step) in the lane order of the skinny fp32 kernels' weight loads.  Expert w_1 [E, F, D] packs as it stands; the slice-major
    w_2 [E, F/S, D, S] gives [E, F/S, D/16, S/16, 4, 16, 4]: the S/16 loads of one output tile are one contiguous run."""
    *lead, N_, K_ = t.shape
    assert N_ % 16 == 0 and K_ % 16 == 0, "pack_wfrag: N=%d and K=%d must be multiples of 16" % (N_, K_)
    n = len(lead)
    v = t.reshape(*lead, N_ // 16, 16, K_ // 16, 4, 4)                       # [.., nt, col, s, kq, j]
    return v.permute(*range(n), n, n + 2, n + 3, n + 1, n + 4).contiguous()  # [.., nt, s, kq, col, j]


def unpack_wfrag(t):
    """inverse of pack_wfrag: [..., N/16, K/16, 4, 16, 4] -> [..., N, K]"""
    *lead, nt, ns, kq, col, j = t.shape
    assert (kq, col, j) == (4, 16, 4)
    n = len(lead)
    return t.permute(*range(n), n, n + 3, n + 1, n + 2, n + 4).reshape(*lead, nt * 16, ns * 16).contiguous()


# the block GEMM weights the skinny fp32 form streams (not the router, out_linear, the convs or the subsampling Linear)
_FRAG_DENSE = ("feed_forward_macaron.w_1.ln.weight", "feed_forward_macaron.w_2.weight", "self_attn.qkv.ln.weight",
               "self_attn.linear_out.weight", "conv_module.pointwise_conv1.ln.weight", "conv_module.pointwise_conv2.weight",
               "feed_forward.w_1.ln.weight", "feed_forward.w_2.weight")


def add_frag_weights(weights, cfg: EncoderConfig):
    """Adds to `weights` (packed names -> tensors, any device) the fragment-ordered copies (pack_wfrag) of the fp32 block GEMM
    weights and expert weights as NAME_frag, beside the tensors they are made from, which every long-batch form keeps reading
    (experts: ...w_1.weight_frag from w_1.weight, ...w_2.weight_frag from w_2.weight_sliced).  fp32 models with attention_dim >=
    256 and cfg.weights_frag only; names already present are kept.  Returns the names added.  save_plan never writes them."""
    if not getattr(cfg, "weights_frag", True) or cfg.weight_dtype != "f32" or cfg.attention_dim < 256:
        return []
    added = []
    for name in list(weights):
        if not (name.startswith("blocks.") or name.startswith("embed.blocks.")):
            continue
        w, dst = weights[name], None
        if w.dtype != torch.float32:
            continue
        if name.endswith(_FRAG_DENSE) and w.dim() == 2 and w.shape[0] % 16 == 0 and w.shape[1] % 16 == 0:
            dst = name + "_frag"
        elif name.endswith("feed_forward.experts.w_1.weight") and w.dim() == 3 and w.shape[1] % 16 == 0 and w.shape[2] % 16 == 0:
            dst = name + "_frag"
        elif name.endswith("feed_forward.experts.w_2.weight_sliced") and w.dim() == 4 and w.shape[2] % 16 == 0 and w.shape[3] % 16 == 0:
            dst = name[:-len("_sliced")] + "_frag"
        if dst is not None and dst not in weights:
            weights[dst] = pack_wfrag(w)
            added.append(dst)
    return added


def _pack_subsampling(sd, p, out):
    w0 = sd[p + "conv.0.weight"]                         # (C,in_ch,3,3) -> [in_ch * 9][C], row ch * 9 + kh * 3 + kw
    C = w0.shape[0]
    out[p + "conv.0.weight_9c"] = w0.reshape(C, w0.shape[1] * 9).t().contiguous()
    out[p + "conv.0.bias"] = sd[p + "conv.0.bias"]
    out[p + "conv.2.weight_ohwi"] = sd[p + "conv.2.weight"].permute(0, 2, 3, 1).contiguous()
    out[p + "conv.2.bias"] = sd[p + "conv.2.bias"]
    wl = sd[p + "out.0.weight"]                          # (D, C*F2), column index c*F2 + f
    F2 = wl.shape[1] // C
    out[p + "out.0.weight"] = wl.view(-1, C, F2).permute(0, 2, 1).reshape(wl.shape[0], F2 * C).contiguous()
    out[p + "out.0.bias"] = sd[p + "out.0.bias"]


def fold_layernorm(weight, bias, gamma, beta):
    """Linear(LayerNorm(x)) = ((x - mean) * rstd) @ (W * gamma)^T + (b + W @ beta): the LayerNorm's affine moves
    into the Linear, so the GEMM prologue only normalises (one fewer dependent load in a latency-bound kernel)."""
    w64, g64, b64 = weight.double(), gamma.double(), beta.double()
    wf = (w64 * g64.unsqueeze(0)).float()
    return {"ln.weight": wf, "ln.bias": (bias.double() + w64 @ b64).float(),
            # output-side LayerNorm (gemm.hip LN_EPI): y = rstd * (x . W'^T - mean * wsum) + bias'
            "ln.wsum": wf.double().sum(1).float(),
            # a frame masked to 0 AFTER the LayerNorm must see the plain bias: bias' - W.beta
            "ln.wbeta": (w64 @ b64).float()}


def _put_folded(out, prefix, folded, keep_wbeta=False):
    for k, v in folded.items():
        if k != "ln.wbeta" or keep_wbeta:
            out[prefix + k] = v


def _pack_block(sd, p, out, norm, moe, cfg):
    folded = ["norm_ff_macaron", "norm_mha", "norm_conv"] + ([] if moe else ["norm_ff"])
    for n in ("norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"):
        if n not in folded:
            out[p + n + ".weight"] = sd[p + n + ".weight"]
            out[p + n + ".bias"] = sd[p + n + ".bias"]
    for n in ("feed_forward_macaron.w_2", "self_attn.linear_out"):
        out[p + n + ".weight"] = sd[p + n + ".weight"]
        out[p + n + ".bias"] = sd[p + n + ".bias"]
    m = p + "feed_forward_macaron.w_1."
    _put_folded(out, m, fold_layernorm(sd[m + "weight"], sd[m + "bias"],
                                       sd[p + "norm_ff_macaron.weight"], sd[p + "norm_ff_macaron.bias"]))
    a = p + "self_attn."
    wqkv = torch.cat([sd[a + "linear_q.weight"], sd[a + "linear_k.weight"], sd[a + "linear_v.weight"]], 0)
    bqkv = torch.cat([sd[a + "linear_q.bias"], sd[a + "linear_k.bias"], sd[a + "linear_v.bias"]], 0)
    _put_folded(out, a + "qkv.", fold_layernorm(wqkv, bqkv, sd[p + "norm_mha.weight"], sd[p + "norm_mha.bias"]))
    out[a + "pos_bias_u"] = sd[a + "pos_bias_u"]
    out[a + "pos_bias_v"] = sd[a + "pos_bias_v"]
    c = p + "conv_module."
    _put_folded(out, c + "pointwise_conv1.",
                fold_layernorm(sd[c + "pointwise_conv1.weight"].squeeze(-1), sd[c + "pointwise_conv1.bias"],
                               sd[p + "norm_conv.weight"], sd[p + "norm_conv.bias"]), keep_wbeta=True)
    out[c + "pointwise_conv2.weight"] = sd[c + "pointwise_conv2.weight"].squeeze(-1)
    out[c + "pointwise_conv2.bias"] = sd[c + "pointwise_conv2.bias"]
    dw = sd[c + "depthwise_conv.weight"].squeeze(1)      # (C, K)
    db = sd[c + "depthwise_conv.bias"]
    if norm == "layer_norm":
        out[c + "norm.weight"] = sd[c + "norm.weight"]
        out[c + "norm.bias"] = sd[c + "norm.bias"]
    else:  # eval BatchNorm1d folds into the depthwise conv: y = (x - mean) / sqrt(var + eps) * g + b
        s = sd[c + "norm.weight"] / torch.sqrt(sd[c + "norm.running_var"] + 1e-5)
        dw = dw * s.unsqueeze(1)
        db = (db - sd[c + "norm.running_mean"]) * s + sd[c + "norm.bias"]
    out[c + "depthwise_conv.weight_kc"] = dw.t().contiguous()
    out[c + "depthwise_conv.bias"] = db
    if (cfg.causal if moe else cfg.embed_causal):
        # causal module (convolution.py:43-49,118-123): lorder = K - 1 ZERO frames are padded in front of pointwise_conv1, so at
        # the depthwise conv's input a frame left of the utterance is the constant GLU(pointwise_conv1.bias)
        b1 = sd[c + "pointwise_conv1.bias"]
        half = b1.numel() // 2
        out[c + "left_fill"] = b1[:half] * torch.sigmoid(b1[half:])
    f = p + "feed_forward."
    if not moe:
        _put_folded(out, f + "w_1.", fold_layernorm(sd[f + "w_1.weight"], sd[f + "w_1.bias"],
                                                    sd[p + "norm_ff.weight"], sd[p + "norm_ff.bias"]))
        out[f + "w_2.weight"] = sd[f + "w_2.weight"]
        out[f + "w_2.bias"] = sd[f + "w_2.bias"]
    else:
        out[f + "router_weights_t"] = sd[f + "router_weights"].t().contiguous()
        # fused route path: the x half of the router with norm_ff folded in (the embed half of all layers is stacked
        # into router_e_all by pack_weights)
        De_ = sd[f + "router_weights"].shape[0] - sd[p + "norm_ff.weight"].shape[0]
        rb = sd[f + "router_bias"] if (f + "router_bias") in sd else torch.zeros(sd[f + "router_weights"].shape[1])
        _put_folded(out, f + "router_x.", fold_layernorm(sd[f + "router_weights"][De_:].t().contiguous(), rb,
                                                         sd[p + "norm_ff.weight"], sd[p + "norm_ff.bias"]))
        if (f + "router_bias") in sd:
            out[f + "router_bias"] = sd[f + "router_bias"]
        if getattr(cfg, "fp8_activations", False) and cfg.weight_dtype == "fp8":
            # static scale of the hidden activations for the fp8-arithmetic expert FFN: from the calibrator
            # (m3asr/calibrate.py writes "...experts.h_scale" into the state dict), else the uncalibrated default
            hs = sd.get(f + "experts.h_scale")
            out[f + "experts.h_scale"] = (hs.reshape(1).float() if hs is not None else torch.tensor([DEFAULT_H_SCALE]))
        lo = cfg.ep_rank * cfg.num_experts if cfg.ep_world_size > 1 else 0
        for n in ("experts.w_1.weight", "experts.w_1.bias", "experts.w_2.weight", "experts.w_2.bias"):
            t = sd[f + n]
            if cfg.ep_world_size > 1 and t.shape[0] == cfg.num_experts * cfg.ep_world_size:
                t = t[lo: lo + cfg.num_experts]
            assert t.shape[0] == cfg.num_experts, "%s: %d experts, config says %d" % (f + n, t.shape[0], cfg.num_experts)
            if n == "experts.w_2.weight":
                out[f + "experts.w_2.weight_sliced"] = slice_major_w2(t)
            else:
                out[f + n] = t


def pack_weights(state_dict, cfg: EncoderConfig):
    """reference-layout state_dict (CPU fp32) -> OrderedDict of packed contiguous fp32 tensors."""
    sd = {k: v.detach().float() for k, v in state_dict.items()}
    out = OrderedDict()
    _pack_subsampling(sd, "embed.subsampling.", out)
    out["embed.after_norm.weight"] = sd["embed.after_norm.weight"]
    out["embed.after_norm.bias"] = sd["embed.after_norm.bias"]
    for i in range(cfg.embed_blocks):
        _pack_block(sd, "embed.blocks.%d." % i, out, cfg.embed_cnn_module_norm, False, cfg)
    _pack_subsampling(sd, "subsampling.", out)
    for i in range(cfg.num_blocks):
        _pack_block(sd, "blocks.%d." % i, out, cfg.cnn_module_norm, True, cfg)
    _put_folded(out, "out_linear.", fold_layernorm(sd["out_linear.weight"], sd["out_linear.bias"],
                                                   sd["after_norm.weight"], sd["after_norm.bias"]))
    out["router_e_all.weight"] = torch.cat(
        [sd["blocks.%d.feed_forward.router_weights" % i][:cfg.embed_dim].t() for i in range(cfg.num_blocks)], 0).contiguous()
    out["pe"] = positional_table(cfg.max_len, cfg.attention_dim)
    # every block's linear_pos weight stacked: p for all blocks = one GEMM per forward (attention.py:345)
    out["pos_all.weight"] = torch.cat(
        [sd["embed.blocks.%d.self_attn.linear_pos.weight" % i] for i in range(cfg.embed_blocks)] +
        [sd["blocks.%d.self_attn.linear_pos.weight" % i] for i in range(cfg.num_blocks)], 0)
    return cast_gemm_weights(OrderedDict((k, v.contiguous()) for k, v in out.items()), cfg)


def memory_norm(state_dict):
    """The encoder's final LayerNorm as vectors, `after_norm.weight` / `after_norm.bias` (pack_weights folds it into out_linear):
    with them in its plan Engine.hidden() can turn the residual stream into the attention decoder's memory."""
    enc = "encoder." if "encoder.after_norm.weight" in state_dict else ""
    return OrderedDict((n, state_dict[enc + n].detach().float().contiguous()) for n in ("after_norm.weight", "after_norm.bias"))


def has_decoder(state_dict, prefix="decoder."):
    """whether a checkpoint carries an attention decoder under `prefix`"""
    return any(k.startswith(prefix) and k.endswith("embed.0.weight") for k in state_dict)


def decoder_config_from_state_dict(state_dict, prefix="decoder.", heads=4, activation="relu"):
    """DecoderConfig of the decoder under `prefix`, from its tensors' shapes (heads and activation are not in the shapes)."""
    bi = (prefix + "left_decoder.embed.0.weight") in state_dict
    left = prefix + ("left_decoder." if bi else "")

    def blocks(p):
        n = 0
        while (p + "decoders.%d.norm1.weight" % n) in state_dict:
            n += 1
        return n

    V, D = state_dict[left + "embed.0.weight"].shape
    F = state_dict[left + "decoders.0.feed_forward.w_1.weight"].shape[0]
    return DecoderConfig(vocab=int(V), dim=int(D), heads=int(heads), linear_units=int(F), num_blocks=blocks(left),
                         r_num_blocks=blocks(prefix + "right_decoder.") if bi else 0, activation=activation)


def pack_decoder(state_dict, dcfg: DecoderConfig, prefix="decoder."):
    """The attention decoder of a reference-layout state_dict (layer/att_decoder.py: `prefix`embed.0 / decoders.N.* /
    after_norm / output_layer, or left_decoder.* / right_decoder.* under it) -> OrderedDict of packed fp32 tensors for
    m3asr.rescore.AttentionRescorer, to be merged into the encoder's packed weights:
      * `decoder.*` the left-to-right decoder, `decoder.right.*` the right-to-left one: embed.weight, per layer the
        self-attention q/k/v fused into qkv [3D, D], the source attention's linear_q, both linear_out, the FFN, norm1-3
        (kept as vectors: they are the GEMMs' LayerNorm prologue), after_norm, output_layer;
      * decoder.src_kv_all: linear_k / linear_v of the source attention of EVERY layer of both decoders stacked to
        [(L + Lr) 2D, D] -- the memory is projected by one GEMM per rescoring call (pos_all.weight is the precedent); layer l
        owns rows [l 2D, l 2D + D) = K and the next D = V, the right decoder's layers follow the left one's;
      * decoder.pe, the sinusoidal table; after_norm.weight / bias: the encoder's final LayerNorm as vectors (pack_weights
        folds it into out_linear), which turns the engine's residual stream into the decoder's memory.
    The decoder's weights stay fp32 whatever the plan's weight_dtype: cast_gemm_weights is not applied to them."""
    sd = {k: v.detach().float() for k, v in state_dict.items()}
    bi = dcfg.r_num_blocks > 0
    out = OrderedDict()
    kv_w, kv_b = [], []
    for src, dst, blocks in ((prefix + ("left_decoder." if bi else ""), "decoder.", dcfg.num_blocks),
                             (prefix + "right_decoder.", "decoder.right.", dcfg.r_num_blocks)):
        if blocks == 0 and dst != "decoder.":
            continue
        emb = sd[src + "embed.0.weight"]
        assert tuple(emb.shape) == (dcfg.vocab, dcfg.dim), "%sembed.0.weight %s, config says (%d, %d)" % (
            src, tuple(emb.shape), dcfg.vocab, dcfg.dim)
        out[dst + "embed.weight"] = emb
        for n in ("after_norm.weight", "after_norm.bias", "output_layer.weight", "output_layer.bias"):
            out[dst + n] = sd[src + n]
        for i in range(blocks):
            p, q = src + "decoders.%d." % i, dst + "layers.%d." % i
            a = p + "self_attn."
            out[q + "self_attn.qkv.weight"] = torch.cat([sd[a + "linear_%s.weight" % n] for n in "qkv"], 0)
            out[q + "self_attn.qkv.bias"] = torch.cat([sd[a + "linear_%s.bias" % n] for n in "qkv"], 0)
            c = p + "src_attn."
            kv_w += [sd[c + "linear_k.weight"], sd[c + "linear_v.weight"]]
            kv_b += [sd[c + "linear_k.bias"], sd[c + "linear_v.bias"]]
            for n in ("self_attn.linear_out", "src_attn.linear_q", "src_attn.linear_out", "feed_forward.w_1", "feed_forward.w_2",
                      "norm1", "norm2", "norm3"):
                out[q + n + ".weight"] = sd[p + n + ".weight"]
                out[q + n + ".bias"] = sd[p + n + ".bias"]
            assert out[q + "feed_forward.w_1.weight"].shape[0] == dcfg.linear_units
    if kv_w:
        out["decoder.src_kv_all.weight"] = torch.cat(kv_w, 0)
        out["decoder.src_kv_all.bias"] = torch.cat(kv_b, 0)
    out["decoder.pe"] = positional_table(dcfg.max_len, dcfg.dim)
    out.update(memory_norm(sd))
    return OrderedDict((k, v.contiguous()) for k, v in out.items())


def decoder_config_of(extra):
    """DecoderConfig a plan's header carries (extra["decoder"]), or None for an encoder-only plan."""
    d = (extra or {}).get("decoder")
    return None if d is None else DecoderConfig.from_dict(d)


def read_cmvn_stats(path):
    """Global CMVN statistics -> (mean, istd) float32 vectors.  Accepts a Kaldi text matrix
    ``[ sum_0 .. sum_{d-1} count \\n sumsq_0 .. sumsq_{d-1} 0 ]`` (what ``Cmvn.read_stats`` loads in
    trainer_3m_fix/loader/cectc_lattice_loader.py:21-24, applied with norm_vars=True) or a 2 x d ``.npy`` of (mean, istd)."""
    if path.endswith(".npy"):
        a = np.load(path, allow_pickle=False).astype(np.float64)
        return torch.from_numpy(a[0].astype(np.float32)), torch.from_numpy(a[1].astype(np.float32))
    txt = open(path).read().replace("[", " ").replace("]", " ")
    vals = np.array([float(v) for v in txt.split()], dtype=np.float64)
    stats = vals.reshape(2, -1)
    count = stats[0, -1]
    mean = stats[0, :-1] / count
    var = np.maximum(stats[1, :-1] / count - mean * mean, 1e-20)
    return torch.from_numpy(mean.astype(np.float32)), torch.from_numpy((1.0 / np.sqrt(var)).astype(np.float32))


def add_front_back_end(packed, cfg, cmvn=None, output_bias=None):
    """Optional front / back end of the acoustic score, attached to a packed weight dict:
    cmvn = (mean, istd) -> fused into the first subsampling conv of both encoders; output_bias [V] (e.g. -log prior,
    builder.py:83-88) -> added after log_softmax when cfg.log_softmax_out, else folded into out_linear's bias."""
    if cmvn is not None:
        packed["cmvn.mean"] = torch.as_tensor(cmvn[0], dtype=torch.float32).contiguous()
        packed["cmvn.istd"] = torch.as_tensor(cmvn[1], dtype=torch.float32).contiguous()
    if output_bias is not None:
        ob = torch.as_tensor(output_bias, dtype=torch.float32).flatten().contiguous()
        assert ob.numel() == cfg.output_dim
        if cfg.log_softmax_out:
            packed["output_bias"] = ob
        else:
            packed["out_linear.ln.bias"] = packed["out_linear.ln.bias"] + ob
    return packed


# GEMM weights that follow cfg.weight_dtype (csrc/engine.hip GETW); everything else -- router, norms, biases,
# conv1, depthwise conv, positional table -- stays fp32 in every mode.
_GEMM_WEIGHT = re.compile(
    r"((feed_forward_macaron|feed_forward)\.w_1|self_attn\.qkv|pointwise_conv1|^out_linear)\.ln\.weight$"
    r"|((feed_forward_macaron|feed_forward)\.w_2|self_attn\.linear_out|pointwise_conv2|subsampling\.out\.0)\.weight$"
    r"|experts\.w_1\.weight$|experts\.w_2\.weight_sliced$|conv\.2\.weight_ohwi$|^pos_all\.weight$")


def is_gemm_weight(name):
    return _GEMM_WEIGHT.search(name) is not None


FP8_MAX = 448.0    # largest finite OCP e4m3 value


# uncalibrated H scale of the fp8-arithmetic expert FFN: |H| up to 448 * 0.05 = 22.4 is representable (H = SiLU(z) of a
# LayerNorm'd input through ~unit-gain weights stays below that); e4m3 is floating point, so a loose scale costs range, not
# precision -- the calibrator (m3asr/calibrate.py) replaces it by 1.25 x the observed maximum / 448
DEFAULT_H_SCALE = 0.05


def quantize_fp8_rows(w, dims):
    """Per-output-row symmetric quantisation to OCP e4m3 (torch.float8_e4m3fn = the format of gfx950's fp8 conversions):
    scale = amax over `dims` / 448, q = round_to_nearest_even(w / scale).  Returns (q fp8, scale fp32 with `dims` removed)."""
    amax = w.abs().amax(dim=dims, keepdim=True).clamp_min(1e-30)
    scale = (amax / FP8_MAX).float()
    q = (w / scale).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous()
    return q, scale.squeeze(dims).contiguous()


MX_BLOCK = 32      # elements per OCP MX block (one e8m0 scale each), along the GEMM's K
_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4(w, dim):
    """OCP MXFP4 along `dim` (the GEMM's K, a multiple of 32): e2m1 elements, one e8m0 scale byte per 32 consecutive elements.
    -> (q uint8, `dim` halved: two codes per byte, the even-k element in the low nibble; scale uint8, `dim` / 32).
    Scale code s = clamp(floor(log2(amax)) - 2, -64, 64) + 127 (the clamp keeps every decoded value a normal bf16 and the code
    away from 0 and 255; an all-zero block stores 127).  Elements: w / 2^(s - 127) rounded to the nearest of
    {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating at +-6; sign in bit 3 (a zero carries none).
    This is the ONE definition of the format: the kernels (csrc/moe_expert_mxfp4.hip) decode exactly this."""
    dim = dim % w.dim()
    K = w.shape[dim]
    assert K % MX_BLOCK == 0, "mxfp4: K = %d must be a multiple of %d" % (K, MX_BLOCK)
    v = w.detach()
    v = (v if v.dtype in (torch.float32, torch.float64) else v.float()).movedim(dim, -1)   # powers of two: exact in either
    blk = v.reshape(*v.shape[:-1], K // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(-1)
    _, ex = torch.frexp(amax)                                  # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = (ex.long() - 3).clamp(-64, 64)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    a = torch.ldexp(blk.abs(), (-e).unsqueeze(-1).expand_as(blk).to(torch.int32))
    # midpoints of neighbouring grid values; a tie goes to the even code
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8) +
            (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = code + (((blk < 0) & (code > 0)).to(torch.uint8) << 3)
    code = code.reshape(*v.shape[:-1], K // 2, 2)
    q = (code[..., 0] | (code[..., 1] << 4)).movedim(-1, dim).contiguous()
    scale = (e + 127).to(torch.uint8).movedim(-1, dim).contiguous()
    return q, scale


def dequantize_mxfp4(q, scale, dim):
    """Inverse of quantize_mxfp4 on its own output: fp32 values (every one exact in bf16), `dim` doubled."""
    dim = dim % q.dim()
    qv, sv = q.movedim(dim, -1), scale.movedim(dim, -1)
    code = torch.stack([qv & 15, qv >> 4], -1).reshape(*qv.shape[:-1], qv.shape[-1] * 2).long()
    mag = torch.tensor(_E2M1_GRID, dtype=torch.float32)[code & 7]
    val = torch.where((code & 8) != 0, -mag, mag)
    ex = (sv.to(torch.int32) - 127).repeat_interleave(MX_BLOCK, -1)
    return torch.ldexp(val, ex).float().movedim(-1, dim).contiguous()


def cast_gemm_weights(packed, cfg: EncoderConfig):
    """Store the GEMM weights in cfg.weight_dtype ("f32" = no-op, "bf16" = round to nearest even).  The reference
    wires --fp16 / plugin_data_type = 1 (builder.py:160, builder_helper.py:47-57,109-123) without finishing it; bf16 is
    the 16-bit type on CDNA4.  "fp8": additionally the expert weights (94 % of the parameters) become e4m3 with one scale per
    output row (W8A16: dequantised to bf16 at the MFMA input); "mxfp4": the expert weights become MXFP4 instead (quantize_mxfp4 along
    each GEMM's K: uint8 code pairs + uint8 scale bytes, W4A16), everything else as in "fp8".  The folded LayerNorm's column sums are recomputed from the ROUNDED weights, so that
    y = rstd * (a . W'^T - mean * wsum) stays an exact identity for the weights the kernel really multiplies by."""
    if cfg.weight_dtype == "f32":
        return packed
    assert cfg.weight_dtype in ("bf16", "fp8", "mxfp4"), cfg.weight_dtype
    out = OrderedDict()
    for k, v in packed.items():
        if cfg.weight_dtype == "mxfp4" and v.dtype == torch.float32 and k.endswith("experts.w_1.weight"):
            out[k], out[k[:-len("weight")] + "scale"] = quantize_mxfp4(v, dim=2)          # [E][F][D/2] + [E][F][D/32]
        elif cfg.weight_dtype == "mxfp4" and v.dtype == torch.float32 and k.endswith("experts.w_2.weight_sliced"):
            # [E][F/64][D][64]: K = F runs along the last axis inside a slice -> [E][F/64][D][32] + [E][F/64][D][2]
            out[k], out[k[:-len("weight_sliced")] + "scale"] = quantize_mxfp4(v, dim=3)
        elif cfg.weight_dtype == "fp8" and v.dtype == torch.float32 and k.endswith("experts.w_1.weight"):
            q, sc = quantize_fp8_rows(v, dims=(2,))                       # [E][F][D]: one scale per (e, f)
            out[k], out[k[:-len("weight")] + "scale"] = q, sc
        elif cfg.weight_dtype == "fp8" and v.dtype == torch.float32 and k.endswith("experts.w_2.weight_sliced"):
            q, sc = quantize_fp8_rows(v, dims=(1, 3))                     # [E][F/64][D][64]: one scale per (e, d)
            out[k], out[k[:-len("weight_sliced")] + "scale"] = q, sc
        elif is_gemm_weight(k) and v.dtype == torch.float32:
            out[k] = v.to(torch.bfloat16).contiguous()
        else:
            out[k] = v
    for k in list(out):
        if k.endswith(".ln.weight") and out[k].dtype == torch.bfloat16:
            out[k[:-len("weight")] + "wsum"] = out[k].double().sum(1).float()
    return out


_DTYPES = {"f32": (torch.float32, "<f4", 4), "bf16": (torch.bfloat16, "<u2", 2), "i32": (torch.int32, "<i4", 4),
           "fp8": (torch.float8_e4m3fn, "u1", 1), "u8": (torch.uint8, "u1", 1)}
_DTYPE_NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.float8_e4m3fn: "fp8", torch.uint8: "u8"}


def save_plan(path, cfg: EncoderConfig, packed, extra=None):
    # (the fragment-ordered copies an Engine derives, NAME_frag, are never written: a plan's bytes do not depend on them)
    packed = {k: v for k, v in packed.items() if not k.endswith("_frag")}
    index, off = {}, 0
    for k, v in packed.items():
        name = _DTYPE_NAME[v.dtype]
        index[k] = [off, list(v.shape)] + ([name] if name != "f32" else [])
        off += (v.numel() * _DTYPES[name][2] + 255) // 256 * 256
    header = json.dumps({"config": json.loads(cfg.to_json()), "tensors": index, "extra": extra or {}}).encode()
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<Q", len(header)))
        f.write(header)
        pad = (-(16 + len(header))) % 256
        f.write(b"\0" * pad)
        for k, v in packed.items():
            if v.dtype == torch.bfloat16:
                b = v.contiguous().view(torch.int16).numpy().astype("<i2", copy=False).tobytes()
            elif v.dtype == torch.float8_e4m3fn:
                b = v.contiguous().view(torch.uint8).numpy().tobytes()
            else:
                b = v.contiguous().numpy().astype(_DTYPES[_DTYPE_NAME[v.dtype]][1], copy=False).tobytes()
            f.write(b)
            f.write(b"\0" * ((-len(b)) % 256))


def load_plan(path):
    """-> (EncoderConfig, OrderedDict name -> CPU tensor (fp32; bf16 for the GEMM weights of a bf16 plan), extra dict)"""
    with open(path, "rb") as f:
        if f.read(8) != MAGIC:
            raise ValueError("%s is not an m3asr plan" % path)
        (hl,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(hl).decode())
    base = 16 + hl
    base += (-base) % 256
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    packed = OrderedDict()
    for k, ent in header["tensors"].items():
        off, shape = ent[0], ent[1]
        tdt, ndt, _ = _DTYPES[ent[2] if len(ent) > 2 else "f32"]
        n = int(np.prod(shape)) if shape else 1
        if tdt == torch.bfloat16:
            arr = np.frombuffer(mm, dtype="<i2", count=n, offset=base + off).reshape(shape)
            packed[k] = torch.from_numpy(np.array(arr, copy=True)).view(torch.bfloat16)
        elif tdt == torch.float8_e4m3fn:
            arr = np.frombuffer(mm, dtype="u1", count=n, offset=base + off).reshape(shape)
            packed[k] = torch.from_numpy(np.array(arr, copy=True)).view(torch.float8_e4m3fn)
        else:
            arr = np.frombuffer(mm, dtype=ndt, count=n, offset=base + off).reshape(shape)
            packed[k] = torch.from_numpy(np.array(arr, copy=True))
    return EncoderConfig(**header["config"]), packed, header.get("extra", {})
