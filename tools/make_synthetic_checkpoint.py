#!/usr/bin/env python3
"""Write a synthetic checkpoint + yaml config in the reference's formats (the real ones are not shipped,
README.md:6,13): ``python tools/make_synthetic_checkpoint.py --out-dir /tmp/m3 [--tiny] [--layers 18] [--decoder-blocks N [--r-decoder-blocks M]]``.
--decoder-blocks adds the attention decoder of a joint CTC/attention model (`decoder.*`; with --r-decoder-blocks a
BiTransformerDecoder's left_decoder / right_decoder).  --add-deltas N: a model trained on the loader's delta features, 40 * (1 + N)
input columns (build it with builder.py --add-deltas N); --in-ch / --embed-in-ch: conv_subsample_in_ch of the main / embed
subsampler (e.g. 3 with --add-deltas 2: static | delta | delta-delta as image channels)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import torch
import yaml

from m3asr.config import DecoderConfig, EncoderConfig
from m3asr.weights import make_decoder_weights, make_weights


def reference_yaml(cfg, dcfg=None):
    y = _encoder_yaml(cfg)
    if dcfg is not None:
        y["model_conf"]["decoder_type"] = "bitransformer" if dcfg.r_num_blocks > 0 else "transformer"
        y["model_conf"]["decoder_conf"] = {"attention_heads": dcfg.heads, "linear_units": dcfg.linear_units,
                                           "num_blocks": dcfg.num_blocks}
        if dcfg.r_num_blocks > 0:
            y["model_conf"]["decoder_conf"]["r_num_blocks"] = dcfg.r_num_blocks
    return y


def _encoder_yaml(cfg):
    y = _encoder_yaml_base(cfg)
    if cfg.conv_subsample_in_ch != 1:
        y["model_conf"]["encoder_conf"]["conv_subsample_in_ch"] = cfg.conv_subsample_in_ch
    if cfg.embed_conv_subsample_in_ch != 1:
        y["model_conf"]["encoder_conf"]["embed_conf"]["conv_subsample_in_ch"] = cfg.embed_conv_subsample_in_ch
    return y


def _encoder_yaml_base(cfg):
    return {"nnet_proto": "conformer_aed_fmoe_localComm_catEmbed_domain_acc_hier", "output_dim": cfg.output_dim,
            "model_conf": {"encoder_conf": {
                "attention_heads": cfg.attention_heads, "attention_dim": cfg.attention_dim, "num_blocks": cfg.num_blocks,
                "cnn_module_kernel": cfg.cnn_module_kernel, "cnn_module_norm": cfg.cnn_module_norm,
                "causal": bool(cfg.causal), "static_chunk_size": int(cfg.static_chunk_size),
                "embed_conf": {"attention_heads": cfg.embed_heads, "attention_dim": cfg.embed_dim,
                               "linear_units": cfg.embed_linear_units, "num_blocks": cfg.embed_blocks,
                               "cnn_module_norm": cfg.embed_cnn_module_norm, "causal": bool(cfg.embed_causal)},
                "moe_conf": {"num_experts": cfg.num_experts, "hidden_units": cfg.hidden_units}}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--decoder-blocks", type=int, default=0, help="add an attention decoder of this many blocks")
    ap.add_argument("--r-decoder-blocks", type=int, default=0, help="and a right-to-left decoder of this many blocks")
    ap.add_argument("--add-deltas", type=int, default=0, help="delta order of the features: 40 * (1 + N) input columns")
    ap.add_argument("--in-ch", type=int, default=1, help="conv_subsample_in_ch of the main encoder's subsampler")
    ap.add_argument("--embed-in-ch", type=int, default=1, help="conv_subsample_in_ch of the embed encoder's subsampler")
    a = ap.parse_args()
    front = dict(input_dim=40 * (1 + a.add_deltas), delta_order=a.add_deltas, conv_subsample_in_ch=a.in_ch,
                 embed_conv_subsample_in_ch=a.embed_in_ch)
    cfg = EncoderConfig.tiny(**front) if a.tiny else EncoderConfig(num_blocks=a.layers, **front)
    os.makedirs(a.out_dir, exist_ok=True)
    sd = {"encoder." + k: v for k, v in make_weights(cfg, seed=a.seed).items()}
    dcfg = None
    if a.decoder_blocks > 0:
        kw = dict(num_blocks=a.decoder_blocks, r_num_blocks=a.r_decoder_blocks)
        dcfg = DecoderConfig.tiny(**kw) if a.tiny else DecoderConfig(vocab=cfg.output_dim, dim=cfg.attention_dim, **kw)
        sd.update(make_decoder_weights(dcfg, seed=a.seed))
    elif a.r_decoder_blocks > 0:
        ap.error("--r-decoder-blocks needs --decoder-blocks")
    torch.save(sd, os.path.join(a.out_dir, "model.pt"))
    with open(os.path.join(a.out_dir, "config.yaml"), "w") as f:
        yaml.safe_dump(reference_yaml(cfg, dcfg), f)
    print("wrote", a.out_dir)


if __name__ == "__main__":
    main()
