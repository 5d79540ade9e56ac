"""CPU tests of what tests/test_stream_kernels_gpu.py holds the streaming kernels to: the references themselves, at the
cases of that file (tests/stream_kernels_ref.py).  No GPU, no library call.

fp32 against fp64: the formula evaluated in fp32 on the CPU stays inside the bound the kernels get (3e-5 / 3e-5 attention,
2e-5 / 2e-5 conv), so a kernel failing its bound fails by its own doing.  The stream restatement against the full-utterance
one: the ring sizes, windows and ragged endings of the cases are consistent before any kernel sees them."""
import pytest
import torch

import stream_kernels_ref as R


def _worst(got, want, rtol, atol):
    """largest error as a fraction of its bound atol + rtol |want|, and the largest absolute error"""
    err = (got.double() - want.double()).abs()
    return float((err / (atol + rtol * want.double().abs())).max()), float(err.max())


@pytest.mark.parametrize("case", R.ATT_CASES + [R.ATT_SLOT_CASE], ids=str)
def test_attention_reference_fp32_within_bound(case):
    d = R.att_inputs(case)
    args = (d.qkv.view(-1, 3 * d.D), d.p, d.u, d.v, d.lens, d.B, d.Ttot, d.H, d.dk, d.C, d.left)
    want = R.attention_ref(*args).view(d.B, d.Ttot, d.D)
    got = R.attention_ref(*args, dtype=torch.float32).view(d.B, d.Ttot, d.D)
    frac, e32 = _worst(got[d.valid], want[d.valid], 3e-5, 3e-5)
    print("attention %s: fp32 CPU max abs err %.3e = %.3f of the 3e-5 / 3e-5 bound" % (case, e32, frac))
    assert frac <= 0.25                                        # the >= 130-key rule of the GPU test (4 x e32) never widens 3e-5 here


@pytest.mark.parametrize("case", R.ATT_CASES + [R.ATT_SLOT_CASE], ids=str)
def test_attention_stream_restatement_matches_full(case):
    d = R.att_inputs(case)
    want = R.attention_ref(d.qkv.view(-1, 3 * d.D), d.p, d.u, d.v, d.lens, d.B, d.Ttot, d.H, d.dk, d.C, d.left).view(d.B, d.Ttot, d.D)
    got, ring = R.attention_stream_ref(d)
    assert bool(torch.isfinite(got).all())                     # the NaN the ring starts with is never read
    err = float((got[d.valid] - want[d.valid]).abs().max())
    print("attention %s: stream restatement vs full, fp64: %.3e" % (case, err))
    assert err <= 1e-12
    m = min(d.cap, d.Ttot)
    f = torch.arange(d.Ttot - m, d.Ttot)
    assert torch.equal(ring[:, f % d.cap], d.qkv[:, f, d.D:].double())


def test_attention_cases_cover_the_grid():
    cs = R.ATT_CASES
    assert {c.dk for c in cs} == {16, 32, 64, 128} and {c.C for c in cs} == {5, 8, 12, 16, 24, 40}
    assert {c.left for c in cs} == {-1, 0, 1, 2} and {c.cap_extra for c in cs if c.left >= 0} == {0, 7, 16}
    assert {c.ldp for c in cs} == {"D+4", "2D"} and {-(-c.C // 16) for c in cs} == {1, 2, 3}
    for c in cs:
        d = R.att_inputs(c)
        last = [int((d.chunk_lens[:, b] > 0).nonzero().max()) for b in range(d.B)]
        assert int(d.chunk_lens[last[1], 1]) == 1 and int(d.chunk_lens[last[2], 2]) == c.C - 1 and last[1] < c.nchunks - 1 and last[2] < c.nchunks - 1


@pytest.mark.parametrize("case", R.CONV_CASES + [R.CONV_SLOT_CASE], ids=str)
def test_conv_reference_fp32_within_bound(case):
    d = R.conv_inputs(case)
    worst = 0.0
    for (want, _), (got, _) in zip(R.conv_stream_ref(d), R.conv_stream_ref(d, dtype=torch.float32)):
        frac, e32 = _worst(got, want, 2e-5, 2e-5)
        worst = max(worst, frac)
    print("conv %s: fp32 CPU worst error %.3f of the 2e-5 / 2e-5 bound" % (case, worst))
    assert worst <= 0.5


@pytest.mark.parametrize("B,T,D,K,ln", [(1, 5, 36, 15, True), (2, 36, 512, 15, True), (7, 99, 32, 7, False), (3, 200, 36, 31, True)])
def test_causal_conv_reference_against_conv1d(B, T, D, K, ln):
    """causal_conv_ref against torch's conv1d on the left-padded sequence (an independent restatement), fp64"""
    import torch.nn.functional as F
    z, fill = R.rnd(B, T, D, seed=1).double(), R.rnd(D, seed=7).double()
    w_kc, bias = R.rnd(K, D, seed=2, scale=0.3), R.rnd(D, seed=3, scale=0.1)
    gamma, beta = (R.rnd(D, seed=4) * 0.2 + 1.0, R.rnd(D, seed=5, scale=0.1)) if ln else (None, None)
    for b in range(B):
        seq = torch.cat([fill.view(1, D).expand(K - 1, D), z[b]])
        y = F.conv1d(seq.t().unsqueeze(0), w_kc.double().t().unsqueeze(1), bias.double(), groups=D)[0].t()
        if ln:
            y = F.layer_norm(y, (D,), gamma.double(), beta.double(), R.CONV_EPS)
        want = y * torch.sigmoid(y)
        assert float((R.causal_conv_ref(seq, w_kc, bias, gamma, beta) - want).abs().max()) <= 1e-12


def test_conv_cases_cover_the_grid():
    cs = R.CONV_CASES
    assert {c.D for c in cs} == {32, 36, 512} and {c.K for c in cs} == {2, 7, 15, 16, 31} and {c.T for c in cs} == {4, 14, 16, 40}
    assert {(c.K > 15, c.ln) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.T > 14) - (c.T < 14) for c in cs if c.K == 15} == {-1, 0, 1}
    d = R.conv_inputs(R.ConvCase(512, 15, 16, True))
    assert sorted(int(d.chunk_lens[:, b][d.chunk_lens[:, b] < 16].max()) for b in range(d.B - 1)) == [1, 13, 14, 15]
    assert bool((d.chunk_lens[-1, :-1] == 0).all()) and bool((d.chunk_lens[:, -1] == 16).all())


def test_next_cache():
    c, z = torch.arange(4.).view(4, 1), torch.arange(10., 16.).view(6, 1)
    assert R.next_cache(c, z, 0).flatten().tolist() == [0, 1, 2, 3]
    assert R.next_cache(c, z, 1).flatten().tolist() == [1, 2, 3, 10]
    assert R.next_cache(c, z, 4).flatten().tolist() == [10, 11, 12, 13]
    assert R.next_cache(c, z, 6).flatten().tolist() == [12, 13, 14, 15]
