"""Host-side checks of attention rescoring: the restated contract (tests/aed_ref.py) against an independent implementation
(torch.nn.TransformerDecoder), the score / selection formula by hand, and the decoder's way through the plan file."""
import math

import pytest
import torch

import aed_ref
from m3asr import _lib
from m3asr.config import DecoderConfig, EncoderConfig
from m3asr.plan import (decoder_config_from_state_dict, decoder_config_of, has_decoder, load_plan, pack_decoder, pack_weights,
                        save_plan)
from m3asr.weights import make_decoder_weights, make_weights


def _nn_decoder(sd, dcfg, prefix="decoder."):
    """torch.nn.TransformerDecoder carrying the same weights (the in-projections concatenated), float64"""
    D = dcfg.dim
    layer = torch.nn.TransformerDecoderLayer(D, dcfg.heads, dcfg.linear_units, dropout=0.0, activation="relu",
                                             layer_norm_eps=1e-12, batch_first=True, norm_first=True)
    dec = torch.nn.TransformerDecoder(layer, dcfg.num_blocks).double().eval()
    new = {}
    for i in range(dcfg.num_blocks):
        p, q = prefix + "decoders.%d." % i, "layers.%d." % i
        for a, b in (("self_attn", "self_attn"), ("src_attn", "multihead_attn")):
            new[q + b + ".in_proj_weight"] = torch.cat([sd[p + a + ".linear_%s.weight" % n] for n in "qkv"], 0)
            new[q + b + ".in_proj_bias"] = torch.cat([sd[p + a + ".linear_%s.bias" % n] for n in "qkv"], 0)
            new[q + b + ".out_proj.weight"] = sd[p + a + ".linear_out.weight"]
            new[q + b + ".out_proj.bias"] = sd[p + a + ".linear_out.bias"]
        for a, b in (("feed_forward.w_1", "linear1"), ("feed_forward.w_2", "linear2"), ("norm1", "norm1"), ("norm2", "norm2"),
                     ("norm3", "norm3")):
            new[q + b + ".weight"] = sd[p + a + ".weight"]
            new[q + b + ".bias"] = sd[p + a + ".bias"]
    dec.load_state_dict({k: v.double() for k, v in new.items()})
    return dec


def test_aed_ref_equals_torch_transformer_decoder():
    """aed_ref's decoder in float64 == torch.nn.TransformerDecoder(norm_first, eps 1e-12, relu) to 1e-10: same weights, same
    embed + pe input, causal and padding masks on a padded batch of three hypotheses over two memory lengths."""
    dcfg = DecoderConfig.tiny()
    sd = {k: v.double() for k, v in make_decoder_weights(dcfg, seed=5).items()}
    g = torch.Generator().manual_seed(1)
    memory = torch.randn(3, 11, dcfg.dim, generator=g, dtype=torch.float64)
    mem_len = [11, 7, 11]
    eos = dcfg.vocab - 1
    hyps = [[3, 1, 4, 1, 5, 9, 2, 6, 5], [], [7]]
    L = max(len(y) for y in hyps) + 1
    dec = _nn_decoder(sd, dcfg)
    tgt = torch.zeros(3, L, dcfg.dim, dtype=torch.float64)
    tgt_pad = torch.ones(3, L, dtype=torch.bool)
    mem_pad = torch.ones(3, 11, dtype=torch.bool)
    for b, y in enumerate(hyps):
        tgt[b, :len(y) + 1] = aed_ref.embed_input(sd, "decoder.", [eos] + y, torch.float64)
        tgt_pad[b, :len(y) + 1] = False
        mem_pad[b, :mem_len[b]] = False
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool), 1)
    with torch.no_grad():
        h = dec(tgt, memory, tgt_mask=causal, tgt_key_padding_mask=tgt_pad, memory_key_padding_mask=mem_pad)
    h = aed_ref.layer_norm(h, sd["decoder.after_norm.weight"], sd["decoder.after_norm.bias"])
    want = torch.log_softmax(h @ sd["decoder.output_layer.weight"].t() + sd["decoder.output_layer.bias"], -1)
    for b, y in enumerate(hyps):
        got = aed_ref.decoder_logp(sd, "decoder.", dcfg.heads, dcfg.num_blocks, "relu", [eos] + y, memory[b, :mem_len[b]])
        err = float((got - want[b, :len(y) + 1]).abs().max())
        print("hypothesis %d: max |aed_ref - nn.TransformerDecoder| = %.3e" % (b, err))
        assert err <= 1e-10


def test_score_and_selection_by_hand():
    """att / r_att / final on a 3-hypothesis example worked out by hand, with the empty hypothesis and a tie"""
    V, eos = 4, 3
    lp = torch.log(torch.tensor([[0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, 0.1], [0.25, 0.25, 0.25, 0.25]], dtype=torch.float64))
    # y = (1, 0): logp[0][1] + logp[1][0] + logp[2][eos]
    assert float(aed_ref.att_score(lp, [1, 0], eos)) == pytest.approx(math.log(0.2) + math.log(0.4) + math.log(0.25), abs=1e-15)
    # the empty hypothesis scores its only row's eos
    assert float(aed_ref.att_score(lp, [], eos)) == pytest.approx(math.log(0.4), abs=1e-15)
    # right-to-left rows are in reversed order: y_0 is read at row n - 1, y_1 at row n - 2
    assert float(aed_ref.r_att_score(lp, [1, 0], eos)) == pytest.approx(math.log(0.3) + math.log(0.1) + math.log(0.25), abs=1e-15)
    t = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    assert float(aed_ref.final_score(t(-2.0), t(-4.0), t(-10.0), 0.5, 0.25)) == pytest.approx(0.75 * -2.0 + 0.25 * -4.0 - 5.0)
    assert float(aed_ref.final_score(t(-2.0), t(-4.0), t(-10.0), 0.0, 0.0)) == -2.0
    assert float(aed_ref.final_score(t(-2.0), t(0.0), t(-float("inf")), 0.0, 0.0)) == -2.0     # an unused prior stays out
    assert aed_ref.select([-3.0, -1.0, -1.0]) == 1            # a tie goes to the earlier n-best position (strict >)
    assert aed_ref.select([-1.0, -3.0, -1.0]) == 0
    assert aed_ref.select([]) == -1


def _checkpoint(r_blocks=0):
    cfg, dcfg = EncoderConfig.tiny(), DecoderConfig.tiny(r_num_blocks=r_blocks)
    sd = {"encoder." + k: v for k, v in make_weights(cfg, seed=2).items()}
    sd.update(make_decoder_weights(dcfg, seed=2))
    return cfg, dcfg, sd


@pytest.mark.parametrize("r_blocks", [0, 1])
def test_pack_decoder_plan_round_trip(tmp_path, r_blocks):
    cfg, dcfg, sd = _checkpoint(r_blocks)
    assert has_decoder(sd) and decoder_config_from_state_dict(sd, heads=dcfg.heads) == dcfg
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    packed = pack_weights(enc, cfg)
    dec = pack_decoder(sd, dcfg)
    D, L = dcfg.dim, dcfg.num_blocks + dcfg.r_num_blocks
    assert tuple(dec["decoder.src_kv_all.weight"].shape) == (L * 2 * D, D)
    left = "decoder." + ("left_decoder." if r_blocks else "")
    assert torch.equal(dec["decoder.src_kv_all.weight"][2 * D + D:2 * D + 2 * D], sd[left + "decoders.1.src_attn.linear_v.weight"])
    assert torch.equal(dec["decoder.layers.0.self_attn.qkv.weight"][D:2 * D], sd[left + "decoders.0.self_attn.linear_k.weight"])
    assert torch.equal(dec["after_norm.weight"], sd["encoder.after_norm.weight"])
    if r_blocks:
        assert torch.equal(dec["decoder.src_kv_all.bias"][dcfg.num_blocks * 2 * D:dcfg.num_blocks * 2 * D + D],
                           sd["decoder.right_decoder.decoders.0.src_attn.linear_k.bias"])
    assert all(v.dtype == torch.float32 for v in dec.values())
    packed.update(dec)
    path = str(tmp_path / "aed.plan")
    save_plan(path, cfg, packed, extra={"decoder": dcfg.to_dict()})
    cfg2, packed2, extra = load_plan(path)
    assert cfg2 == cfg and decoder_config_of(extra) == dcfg
    assert list(packed2) == list(packed)
    assert all(torch.equal(packed2[k], packed[k]) for k in packed)


def test_plan_without_decoder_still_loads_and_is_refused(tmp_path):
    """an encoder-only plan (no extra["decoder"]) loads as before; AttentionRescorer says what is missing"""
    from m3asr.rescore import AttentionRescorer
    cfg = EncoderConfig.tiny()
    packed = pack_weights(make_weights(cfg, seed=2), cfg)
    path = str(tmp_path / "enc.plan")
    save_plan(path, cfg, packed, extra={"profiles": {}})
    cfg2, packed2, extra = load_plan(path)
    assert cfg2 == cfg and list(packed2) == list(packed) and not any(k.startswith("decoder.") for k in packed2)
    assert decoder_config_of(extra) is None
    with pytest.raises(_lib.M3Error, match="no attention decoder"):
        AttentionRescorer(packed2, decoder_config_of(extra), device="cpu")
    with pytest.raises(_lib.M3Error, match="no attention decoder"):
        AttentionRescorer(packed2, DecoderConfig.tiny(), device="cpu")


def test_decoder_config_checks():
    with pytest.raises(ValueError):
        DecoderConfig(activation="gelu")
    with pytest.raises(ValueError):
        DecoderConfig(dim=30, heads=4)
    d = DecoderConfig()
    assert (d.heads, d.linear_units, d.num_blocks, d.r_num_blocks, d.activation) == (4, 2048, 6, 0, "relu")
    assert d.sos == d.eos == d.vocab - 1 and DecoderConfig.from_dict(d.to_dict()) == d
