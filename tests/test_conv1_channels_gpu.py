"""The subsamplers' first conv with input channels (conv1_relu_kernel<IN_CH>, m3_subsample_conv1_ch / _ch_pair) against
torch.nn.functional.conv2d in float64 on the (B, in_ch, T, Fc) view of the frames.

Bound: an output is the bias plus 9 * in_ch fmas in fp32: (9 in_ch + 3) * 2^-24 * (|b| + sum |w x|) -- one rounding per fma,
slack 3; the reference computes that sum per element with the absolute weights and inputs.  CMVN is applied beforehand in
float32 with the kernel's arithmetic ((x - mean) * istd, two roundings), so it is exact in the reference's input.  A bf16
output adds its rounding, 2^-8 relative (bf16 keeps 8 significant bits, so an ulp is 2^-7 of the binade's base and
round-to-nearest moves a value by at most half of that, 2^-8 of the base <= 2^-8 of the value; the worst cases stand close to
it).  Identities are torch.equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from m3asr import _lib, ops

U = 2.0 ** -24


def _problem(B, T, Fc, in_ch, C, seed, cmvn=False):
    g = torch.Generator().manual_seed(seed)
    idim = in_ch * Fc
    feat = torch.randn(B, T, idim, generator=g) * 2 + 0.5
    w = torch.randn(C, in_ch, 3, 3, generator=g) / 3
    b = torch.randn(C, generator=g)
    mv = (torch.randn(idim, generator=g), torch.rand(idim, generator=g) + 0.5) if cmvn else None
    return feat, w, b, mv


def _pack(w):
    return w.reshape(w.shape[0], w.shape[1] * 9).t().contiguous()


def _reference(feat, w, b, mv, in_ch, relu=True):
    """(want, mag) in float64, channel-last (B, T1, F1, C)"""
    x = feat if mv is None else (feat - mv[0].view(1, 1, -1)) * mv[1].view(1, 1, -1)      # float32, as the kernel does
    B, T, idim = x.shape
    x4 = x.double().view(B, T, in_ch, idim // in_ch).transpose(1, 2)
    y = F.conv2d(x4, w.double(), b.double(), stride=2)
    mag = F.conv2d(x4.abs(), w.double().abs(), b.double().abs(), stride=2)
    if relu:
        y = y.clamp(min=0)
    return y.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def _kw(feat, w, b, mv, in_ch, **more):
    d = dict(feat=feat.cuda(), w9c=_pack(w).cuda(), bias=b.cuda(), in_ch=in_ch, **more)
    if mv is not None:
        d["cmvn"] = (mv[0].cuda(), mv[1].cuda())
    return d


def _assert_close(got, want, mag, in_ch, what):
    bf16 = got.dtype == torch.bfloat16
    err = (got.double().cpu() - want).abs()
    bound = (9 * in_ch + 3) * U * mag + (2.0 ** -8 * want.abs() if bf16 else 0)
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("%s: worst err / bound %.3f" % (what, ratio))
    assert tuple(got.shape) == tuple(want.shape) and bool((err <= bound).all()), (what, ratio)


@pytest.mark.parametrize("in_ch", [2, 3])
@pytest.mark.parametrize("Fc,C", [(7, 32), (40, 256), (7, 256), (40, 32)])
def test_single_against_conv2d(in_ch, Fc, C):
    for T, B, cmvn, bf16 in ((3, 2, False, False), (4, 1, True, True), (23, 3, True, False), (23, 1, False, True)):
        feat, w, b, mv = _problem(B, T, Fc, in_ch, C, 1000 * in_ch + 10 * Fc + T, cmvn)
        got = ops.subsample_conv1_ch(**_kw(feat, w, b, mv, in_ch, out_bf16=bf16))
        torch.cuda.synchronize()
        want, mag = _reference(feat, w, b, mv, in_ch)
        assert got.shape[2] == (Fc - 3) // 2 + 1
        _assert_close(got, want, mag, in_ch, "in_ch %d Fc %d C %d T %d cmvn %d bf16 %d" % (in_ch, Fc, C, T, cmvn, bf16))
    # the convolution alone (what network_helper.addConv2d asks for)
    feat, w, b, mv = _problem(2, 5, Fc, in_ch, C, 77)
    got = ops.subsample_conv1_ch(**_kw(feat, w, b, mv, in_ch, act=_lib.ACT_NONE))
    want, mag = _reference(feat, w, b, mv, in_ch, relu=False)
    _assert_close(got, want, mag, in_ch, "no relu")
    assert float(got.min()) < 0


@pytest.mark.parametrize("B,T,Fc,C,in_ch", [(3, 23, 7, 32, 3),        # B * T1 = 33 rows: columns split 5 ways
                                            (4, 259, 7, 256, 2),     # 516 rows: split 2 ways
                                            (16, 259, 7, 32, 3)])    # 2064 rows: no split
def test_column_splits_and_the_fused_lengths(B, T, Fc, C, in_ch):
    feat, w, b, mv = _problem(B, T, Fc, in_ch, C, B + T, cmvn=True)
    assert B * ((T - 3) // 2 + 1) in (33, 516, 2064)
    flen = torch.randint(7, T + 1, (B,), dtype=torch.int32)                       # (7 frames: the shortest utterance with an output frame)
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    got = ops.subsample_conv1_ch(**_kw(feat, w, b, mv, in_ch, feat_len=flen.cuda(), lens_out=lens))
    plain = ops.subsample_conv1_ch(**_kw(feat, w, b, mv, in_ch))
    torch.cuda.synchronize()
    assert lens.cpu().tolist() == [((int(n) - 3) // 2 + 1 - 3) // 2 + 1 for n in flen]
    assert torch.equal(got, plain)
    want, mag = _reference(feat, w, b, mv, in_ch)
    _assert_close(got, want, mag, in_ch, "rows %d" % (B * ((T - 3) // 2 + 1)))


@pytest.mark.parametrize("in_ch", [2, 3])
@pytest.mark.parametrize("T,B", [(3, 1), (4, 3), (23, 2)])
def test_pair(in_ch, T, B):
    """two problems of unequal C (and one with CMVN, one without; fp32 and bf16 out) in one launch == each alone"""
    Fc = 7 if T != 23 else 40
    feat, wa, ba, mv = _problem(B, T, Fc, in_ch, 32, 5 + T, cmvn=True)
    _, wb, bb, _ = _problem(B, T, Fc, in_ch, 256, 6 + T)
    flen = torch.full((B,), T, dtype=torch.int32, device="cuda")
    lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    for bf16 in (False, True):
        ka = _kw(feat, wa, ba, mv, in_ch, out_bf16=bf16, feat_len=flen, lens_out=lens)
        kb = _kw(feat, wb, bb, None, in_ch, out_bf16=bf16)
        oa, ob = ops.subsample_conv1_ch_pair(ka, kb)
        torch.cuda.synchronize()
        assert lens.cpu().tolist() == [((T - 3) // 2 + 1 - 3) // 2 + 1] * B
        ka.pop("feat_len"), ka.pop("lens_out")
        assert torch.equal(oa, ops.subsample_conv1_ch(**ka)) and torch.equal(ob, ops.subsample_conv1_ch(**kb))
        for got, (w, b, m) in ((oa, (wa, ba, mv)), (ob, (wb, bb, None))):
            want, mag = _reference(feat, w, b, m, in_ch)
            _assert_close(got, want, mag, in_ch, "pair in_ch %d T %d bf16 %d" % (in_ch, T, bf16))


def test_one_channel_through_the_new_entry_is_the_old_kernel():
    """in_ch = 1 through m3_subsample_conv1_ch equals m3_subsample_conv1_cmvn / m3_conv2d_3x3s2_first bit for bit"""
    for B, T, idim, C, cmvn in ((2, 23, 40, 256, True), (1, 4, 7, 32, False), (3, 9, 23, 64, True)):
        feat, w, b, mv = _problem(B, T, idim, 1, C, 31 + T, cmvn)
        kw = _kw(feat, w, b, mv, 1)
        new = ops.subsample_conv1_ch(**kw)
        if cmvn:
            old = ops.subsample_conv1_cmvn(kw["feat"], kw["w9c"], kw["bias"], kw["cmvn"])
        else:
            old = ops.subsample_conv1(kw["feat"], kw["w9c"], kw["bias"])
        assert torch.equal(new, old) and float(new.abs().max()) > 0


@pytest.mark.parametrize("C", [32, 256])
def test_zero_weight_channels_are_the_one_channel_problem(C):
    """in_ch = 3 with zero weights on channels 1 and 2 == the in_ch = 1 problem on columns [0, Fc): the extra fmas add +-0 products
    of finite inputs to a running sum, which leaves it as it is"""
    B, T, Fc = 2, 23, 16
    feat, w, b, mv = _problem(B, T, Fc, 3, C, 9, cmvn=True)
    w[:, 1:] = 0
    three = ops.subsample_conv1_ch(**_kw(feat, w, b, mv, 3))
    one = ops.subsample_conv1_ch(**_kw(feat[..., :Fc].contiguous(), w[:, :1].contiguous(), b, (mv[0][:Fc], mv[1][:Fc]), 1))
    assert torch.equal(three, one) and float(one.abs().max()) > 0


def test_refusals():
    feat, w, b, mv = _problem(2, 9, 8, 3, 32, 1)
    _, w1, b1, _ = _problem(2, 9, 24, 1, 32, 2)
    with pytest.raises(_lib.M3Error, match="in_ch"):                              # a pair needs one in_ch
        ops.subsample_conv1_ch_pair(_kw(feat, w, b, None, 3), _kw(feat, w1, b1, None, 1))
    with pytest.raises(_lib.M3Error, match=r"in_ch=4"):
        ops.subsample_conv1_ch(**_kw(feat, torch.zeros(32, 4, 3, 3), b, None, 4))
    with pytest.raises(_lib.M3Error, match="multiple of in_ch"):
        ops.subsample_conv1_ch(**_kw(feat[..., :23].contiguous(), w, b, None, 3))
    with pytest.raises(_lib.M3Error, match="shorter than the 3x3 kernel"):
        ops.subsample_conv1_ch(**_kw(feat[..., :6].contiguous(), w, b, None, 3, out=torch.empty(2, 4, 1, 32, device="cuda")))   # Fc = 2
    torch.cuda.synchronize()
