"""Restatement of the attention-rescoring contract in plain torch, float64-capable (the checker of m3asr.rescore; nothing
here is used by the product; it runs on whatever device its tensors are on).  Written from the reference's text, trainer_3m_fix:

  layer/att_decoder.py:63-142     DecoderLayer.forward, normalize_before=True, concat_after=False:
                                    x += SelfAttn(LN1 x)  (causal, within the hypothesis)
                                    x += SrcAttn(LN2 x, memory)  (keys < mem_len of the hypothesis's utterance)
                                    x += W2 act(W1 LN3 x)
  layer/att_decoder.py:212-256    embed -> layers -> after_norm -> output_layer
  layer/attention.py:136-197      q k^T / sqrt(dk); masked keys -> -inf -> softmax -> masked to 0; linear_out
  layer/positional_encoding.py    x * sqrt(D) + pe[pos], positions from 0
  model/ctc_aed.py:33-34,203-252  sos = eos = V - 1; input [sos, y]; att = sum_j logp[j][y_j] + logp[n][eos]; the right-to-left
                                  decoder reads [sos, reversed y] and r_att = sum_j r_logp[n-1-j][y_j] + r_logp[n][eos];
                                  final = (1 - rw) att + rw r_att + ctc_weight prior; the first strictly largest final wins.

The decoder's feed-forward activation is ReLU (PositionwiseFeedForward's default, which att_decoder.py:204 takes).  All LayerNorms
have eps 1e-12.  Every hypothesis is evaluated alone, unpadded: that is what the masks of the padded reference leave of it.

State-dict layout: the reference's (`decoder.embed.0.weight`, `decoder.decoders.N.self_attn.linear_q.weight`, ...; with a
right-to-left decoder `decoder.left_decoder.*` / `decoder.right_decoder.*`)."""
import math

import torch

EPS = 1e-12


def positional_table(max_len, d, dtype=torch.float64):
    """positional_encoding.py:40-48, built in float32 as the reference does and then cast"""
    pe = torch.zeros(max_len, d)
    position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.to(dtype)


def layer_norm(x, w, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * w + b


def linear(x, sd, p):
    return x @ sd[p + "weight"].t() + sd[p + "bias"]


def attention(sd, p, heads, query, key, visible):
    """MultiHeadedAttention.forward: query (n, D), key = value (m, D), visible (n, m) bool."""
    n, D = query.shape
    dk = D // heads
    q = linear(query, sd, p + "linear_q.").view(n, heads, dk).transpose(0, 1)
    k = linear(key, sd, p + "linear_k.").view(-1, heads, dk).transpose(0, 1)
    v = linear(key, sd, p + "linear_v.").view(-1, heads, dk).transpose(0, 1)
    scores = q @ k.transpose(1, 2) / math.sqrt(dk)
    hidden = ~visible.unsqueeze(0)
    attn = torch.softmax(scores.masked_fill(hidden, -float("inf")), dim=-1).masked_fill(hidden, 0.0)
    return linear((attn @ v).transpose(0, 1).reshape(n, D), sd, p + "linear_out.")


def activation(name):
    return {"relu": torch.relu, "silu": torch.nn.functional.silu}[name]


def embed_input(sd, p, tokens_in, dtype):
    """embed.0 + PositionalEncoding on the (n + 1,) input tokens"""
    emb = sd[p + "embed.0.weight"]
    D = emb.shape[1]
    tok = torch.as_tensor(tokens_in, dtype=torch.long, device=emb.device)
    return emb[tok] * math.sqrt(D) + positional_table(len(tokens_in), D, dtype).to(emb.device)


def decoder_logp(sd, p, heads, blocks, act, tokens_in, memory):
    """One TransformerDecoder under prefix p on one hypothesis: tokens_in = [sos, ...] (n + 1), memory (m, D) the valid
    frames of its utterance -> log_softmax of the output layer, (n + 1, V)."""
    dtype = memory.dtype
    x = embed_input(sd, p, tokens_in, dtype)
    n = x.shape[0]
    causal = torch.tril(torch.ones(n, n, dtype=torch.bool, device=x.device))
    every = torch.ones(n, memory.shape[0], dtype=torch.bool, device=x.device)
    f = activation(act)
    for i in range(blocks):
        q = p + "decoders.%d." % i
        y = layer_norm(x, sd[q + "norm1.weight"], sd[q + "norm1.bias"])
        x = x + attention(sd, q + "self_attn.", heads, y, y, causal)
        y = layer_norm(x, sd[q + "norm2.weight"], sd[q + "norm2.bias"])
        x = x + attention(sd, q + "src_attn.", heads, y, memory, every)
        y = layer_norm(x, sd[q + "norm3.weight"], sd[q + "norm3.bias"])
        x = x + linear(f(linear(y, sd, q + "feed_forward.w_1.")), sd, q + "feed_forward.w_2.")
    x = layer_norm(x, sd[p + "after_norm.weight"], sd[p + "after_norm.bias"])
    return torch.log_softmax(linear(x, sd, p + "output_layer."), dim=-1)


def att_score(logp, y, eos):
    """ctc_aed.py:236-239, summed left to right"""
    s = logp.new_zeros(())
    for j, w in enumerate(y):
        s = s + logp[j][w]
    return s + logp[len(y)][eos]


def r_att_score(r_logp, y, eos):
    """ctc_aed.py:242-245"""
    s = r_logp.new_zeros(())
    for j, w in enumerate(y):
        s = s + r_logp[len(y) - j - 1][w]
    return s + r_logp[len(y)][eos]


def final_score(att, r_att, prior, ctc_weight, reverse_weight):
    """ctc_aed.py:241-248"""
    score = att
    if reverse_weight > 0:
        score = score * (1 - reverse_weight) + r_att * reverse_weight
    if ctc_weight != 0:
        score = score + prior * ctc_weight
    return score


def select(finals):
    """ctc_aed.py:233-251: the first strictly largest; -1 for an utterance without hypotheses"""
    best, best_score = -1, -float("inf")
    for i, s in enumerate(finals):
        if best < 0 or s > best_score:
            best, best_score = i, s
    return best


def rescore(sd, dcfg, memory, mem_len, nbest, ctc_weight=0.0, reverse_weight=0.0, dtype=torch.float64, prefix="decoder."):
    """memory (B, T, D) normalised encoder states, mem_len (B,), nbest [[(tokens, prior)]] per utterance ->
    [dict(att=[..], r_att=[..], final=[..], best=index or -1)] per utterance, as Python floats."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    bi = dcfg.r_num_blocks > 0
    left = prefix + ("left_decoder." if bi else "")
    eos = dcfg.vocab - 1
    assert reverse_weight == 0 or bi, "reverse_weight > 0 needs a right-to-left decoder"
    out = []
    for b, hyps in enumerate(nbest):
        mem = memory[b, :int(mem_len[b])].to(dtype)
        att, r_att, final = [], [], []
        for y, prior in hyps:
            y = [int(t) for t in y]
            a = att_score(decoder_logp(sd, left, dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + y, mem), y, eos)
            r = a.new_zeros(())
            if reverse_weight > 0:
                r = r_att_score(decoder_logp(sd, prefix + "right_decoder.", dcfg.heads, dcfg.r_num_blocks, dcfg.activation,
                                             [eos] + y[::-1], mem), y, eos)
            att.append(float(a))
            r_att.append(float(r))
            final.append(float(final_score(a, r, torch.as_tensor(prior, dtype=dtype, device=a.device), ctc_weight, reverse_weight)))
        out.append(dict(att=att, r_att=r_att, final=final, best=select(final)))
    return out
