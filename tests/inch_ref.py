"""encoder_forward of oracle/encoder_ref.py restated for subsamplers with input channels (conv_subsample_in_ch of the
reference, layer/subsampling.py:23-36): BaseSubsampling.trans_3d_to_4d views (B, T, idim) as (B, T, in_ch, idim / in_ch) and
transposes to (B, in_ch, T, idim / in_ch), the image Conv2d(in_ch, odim, 3, 2) reads.  Everything behind the subsamplers is the
oracle's own code, called, not copied.  Test-side only."""
import torch
import torch.nn.functional as F

from oracle.encoder_ref import conformer_block, layer_norm, rel_pos_enc, sub_len


def trans_3d_to_4d(feat, in_ch):
    b, t, idim = feat.shape
    return feat.view(b, t, in_ch, idim // in_ch).transpose(1, 2)


def subsample(feat, w, p, dtype=torch.float32):
    """Conv2dSubsampling4.forward with in_ch read off the first conv's weight (C, in_ch, 3, 3)"""
    w0 = w[p + "conv.0.weight"]
    x = trans_3d_to_4d(feat.to(dtype), int(w0.shape[1]))
    x = F.relu(F.conv2d(x, w0.to(dtype), w[p + "conv.0.bias"].to(dtype), stride=2))
    x = F.relu(F.conv2d(x, w[p + "conv.2.weight"].to(dtype), w[p + "conv.2.bias"].to(dtype), stride=2))
    b, c, t, f = x.shape
    x = x.transpose(1, 2).contiguous().view(b, t, c * f)
    return F.linear(x, w[p + "out.0.weight"].to(dtype), w[p + "out.0.bias"].to(dtype))


def encoder_forward(w, cfg, feat, feat_len):
    """oracle.encoder_ref.encoder_forward, line for line, with the subsample above -> logits (B, T', V)"""
    feat = feat.float()
    lens = sub_len(feat_len.reshape(-1).to(torch.int64))
    with torch.no_grad():
        x = subsample(feat, w, "embed.subsampling.")
        x, pos = rel_pos_enc(x)
        for i in range(cfg.embed_blocks):
            x = conformer_block(x, None, lens, pos, w, "embed.blocks.%d." % i, cfg, cfg.embed_heads, cfg.cnn_module_kernel,
                                cfg.embed_cnn_module_norm, False, None, "embed.%d." % i)
        embed = layer_norm(x, w, "embed.after_norm.", 1e-12)
        x = subsample(feat, w, "subsampling.")
        x, pos = rel_pos_enc(x)
        for i in range(cfg.num_blocks):
            x = conformer_block(x, embed, lens, pos, w, "blocks.%d." % i, cfg, cfg.attention_heads, cfg.cnn_module_kernel,
                                cfg.cnn_module_norm, True, None, "blocks.%d." % i, None)
        x = layer_norm(x, w, "after_norm.", 1e-12)
        return F.linear(x, w["out_linear.weight"], w["out_linear.bias"])
