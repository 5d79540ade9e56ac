"""References, cases and inputs shared by the kernel-level streaming tests (test-side only; launches nothing).

  attention_ref          the rel-pos attention core with padding and static chunk mask, in any dtype (float64 = the reference of
                         test_strided_operands_gpu.py and test_stream_kernels_gpu.py; float32 = the error of the formula itself)
  attention_stream_ref   the same rows computed the way a stream computes them: chunk by chunk from a K / V ring of `cap` frames
                         indexed by (absolute frame) % cap.  test_stream_kernels_host.py holds it against attention_ref, so the
                         ring sizes, windows and ragged endings the GPU test drives are known to be consistent on their own.
  causal_conv_ref        causal depthwise conv + LayerNorm + SiLU of one utterance [left frames | frames]
  AttCase / ConvCase     the cases of tests/test_stream_kernels_gpu.py with their inputs, so that the host test evaluates the
                         references at exactly the shapes the kernels are held to
"""
import math
from collections import namedtuple

import torch


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _r16(t):
    return t.float().to(torch.bfloat16).double()


def attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk=0, left=-1, round_q16=False, dtype=torch.float64):
    D = H * dk
    q, k, vv = [t.to(dtype).view(B, T, H, dk) for t in qkv.view(B, T, 3 * D).split(D, -1)]
    pp = p.to(dtype).view(1, T, H, dk)
    qu, qv = q + u.to(dtype), q + v.to(dtype)
    if round_q16:
        qu, qv = _r16(qu), _r16(qv)
    ac = torch.matmul(qu.transpose(1, 2), k.permute(0, 2, 3, 1))
    bd = torch.matmul(qv.transpose(1, 2), pp.permute(0, 2, 3, 1))
    hide = (torch.arange(T).view(1, 1, 1, T) >= L.view(B, 1, 1, 1)).expand(B, 1, T, T).clone()
    if chunk > 0:
        i, j = torch.arange(T).view(T, 1), torch.arange(T).view(1, T)
        c = i // chunk
        lo = torch.zeros_like(c) if left < 0 else ((c - left) * chunk).clamp(min=0)
        hide |= ((j < lo) | (j >= (c + 1) * chunk)).view(1, 1, T, T)
    att = torch.softmax(((ac + bd) / math.sqrt(dk)).masked_fill(hide, -float("inf")), -1)
    att = torch.nan_to_num(att, nan=0.0).masked_fill(hide, 0.0)          # a row with no visible key: zeros
    return torch.matmul(att, vv.transpose(1, 2)).transpose(1, 2).reshape(B * T, D)


# ================================================================================================ streaming attention
# dk, C (chunk), left (left chunks), cap_extra (ring frames beyond (left + 1) C; ignored for left < 0: cap = Ttot), ldp ("D+4" or
# "2D", the engine's shared pbuf), nchunks.  H = 2, B = 3 everywhere.  Together: every head width; C = 5 .. 40 (one, two and
# three 16-query tiles; chunk starts on and off multiples of 16 and 4); every `left`; rings of exactly (left + 1) C frames, 7
# more (the ring wraps in the middle of a chunk and of a 16-key tile) and 16 more; every ring wraps at least twice
# (Ttot >= 3 cap, asserted in att_inputs).
AttCase = namedtuple("AttCase", "dk C left cap_extra ldp nchunks")
ATT_CASES = [AttCase(16, 5, 2, 7, "D+4", 14), AttCase(32, 8, 1, 16, "2D", 12), AttCase(64, 12, 0, 0, "D+4", 5),
             AttCase(128, 16, -1, 0, "2D", 6), AttCase(64, 24, 1, 7, "D+4", 7), AttCase(128, 40, 1, 7, "2D", 7),
             AttCase(16, 24, 2, 0, "2D", 9), AttCase(32, 40, 0, 16, "D+4", 5)]
ATT_SLOT_CASE = AttCase(32, 24, 1, 7, "D+4", 8)
ATT_H, ATT_B = 2, 3

AttInputs = namedtuple("AttInputs", "B C H dk D left cap Ttot nchunks ldp qkv p u v lens chunk_lens valid")


def att_inputs(case):
    """Full-sequence operands of a case.  Utterance 0 fills every chunk; utterance 1 ends in a partial chunk of ONE frame,
    utterance 2 in a partial chunk of C - 1 frames; both then get chunk_len = 0 while utterance 0 continues.  qkv holds
    finite random rows for every frame of every utterance (rows at and past a length are what the kernel's contract calls
    finite values), inputs distributed as in test_relpos_attention."""
    dk, C, left, cap_extra, ldp, n = case
    H, B = ATT_H, ATT_B
    D, Ttot = H * dk, n * C
    cap = Ttot if left < 0 else (left + 1) * C + cap_extra
    assert left < 0 or Ttot >= 3 * cap, "the ring must wrap at least twice"
    e1, e2 = n // 2, n - 2                                   # chunk numbers of the two partial endings
    lens = torch.tensor([Ttot, e1 * C + 1, e2 * C + C - 1], dtype=torch.int32)
    chunk_lens = torch.stack([(lens - c * C).clamp(0, C) for c in range(n)]).to(torch.int32)      # [nchunks][B]
    qkv, p = rnd(B, Ttot, 3 * D, seed=1), rnd(Ttot, D, seed=2)
    u, v = rnd(H, dk, seed=3, scale=0.3), rnd(H, dk, seed=4, scale=0.3)
    valid = torch.arange(Ttot).view(1, -1) < lens.view(-1, 1)                                     # [B][Ttot]
    return AttInputs(B, C, H, dk, D, left, cap, Ttot, n, (D + 4 if ldp == "D+4" else 2 * D), qkv, p, u, v, lens, chunk_lens, valid)


def attention_stream_ref(d, dtype=torch.float64):
    """Rows [B][Ttot][D] as a stream forms them (see the module docstring): every chunk appends its C rows (valid or not) of
    K | V to ring slot (frame % cap) AFTER its own keys were taken from the chunk, and reads the frames left of the chunk from
    the ring.  Also returns the ring [B][cap][2 D] after the last chunk."""
    B, C, H, dk, D = d.B, d.C, d.H, d.dk, d.D
    ring = torch.full((B, d.cap, 2 * D), float("nan"), dtype=dtype)
    out = torch.zeros(B, d.Ttot, D, dtype=dtype)
    u, v, p = d.u.to(dtype), d.v.to(dtype), d.p.to(dtype).view(d.Ttot, H, dk)
    for n in range(d.nchunks):
        off = n * C
        for b in range(B):
            nl = int(d.chunk_lens[n, b])
            lo, hi = (0 if d.left < 0 else max((n - d.left) * C, 0)), off + nl
            rows = d.qkv[b, off:off + C].to(dtype)
            keys = [ring[b, j % d.cap] if j < off else rows[j - off, D:] for j in range(lo, hi)]
            if keys:
                kv = torch.stack(keys).view(hi - lo, 2, H, dk)
                q = rows[:, :D].view(C, H, dk)
                s = (torch.einsum("chd,jhd->hcj", q + u, kv[:, 0]) + torch.einsum("chd,jhd->hcj", q + v, p[lo:hi])) / math.sqrt(dk)
                out[b, off:off + C] = torch.einsum("hcj,jhd->chd", torch.softmax(s, -1), kv[:, 1]).reshape(C, D)
        for b in range(B):
            for r in range(C):
                ring[b, (off + r) % d.cap] = d.qkv[b, off + r, D:].to(dtype)
    return out, ring


# ================================================================================================ streaming causal conv
# D, K, T (frames per chunk), ln (LayerNorm or not).  K <= 15 is the one-round kernel (KT = 15), K > 15 the two-round one
# (KT = 8); for K = 15 the chunk is shorter than (T = 4), equal to (T = 14) and longer than (T = 16, 40) the cache.
ConvCase = namedtuple("ConvCase", "D K T ln")
CONV_CASES = [ConvCase(36, 15, 4, True), ConvCase(32, 15, 14, False), ConvCase(512, 15, 16, True), ConvCase(36, 15, 40, False),
              ConvCase(32, 2, 4, True), ConvCase(36, 7, 16, False), ConvCase(32, 16, 14, True), ConvCase(512, 31, 40, False),
              ConvCase(36, 31, 16, True)]
CONV_SLOT_CASE = ConvCase(32, 15, 16, True)
CONV_NCHUNKS = 4
CONV_EPS = 1e-5

ConvInputs = namedtuple("ConvInputs", "B T D K z w_kc bias gamma beta R fill chunk_lens")


def conv_inputs(case, broadcast_fill=False, nchunks=CONV_NCHUNKS):
    """z [nchunks][B][T][D] (rows at and past chunk_len: finite random), the initial cache R [B][K-1][D] (random, or every
    row = `fill` when broadcast_fill), and chunk_lens [nchunks][B]: one utterance per ending e in {1, K-2, K-1, T-1} (those
    within 1 .. T), alternately in chunk 1 and chunk 2, followed by chunk_len = 0; the last utterance fills every chunk."""
    D, K, T, ln = case
    ends = sorted(e for e in {1, K - 2, K - 1, T - 1} if 1 <= e <= T)
    B = len(ends) + 1
    cl = torch.full((nchunks, B), T, dtype=torch.int32)
    for b, e in enumerate(ends):
        at = 1 + (b & 1)
        cl[at, b] = e
        cl[at + 1:, b] = 0
    z = rnd(nchunks, B, T, D, seed=1)
    w_kc, bias = rnd(K, D, seed=2, scale=0.3), rnd(D, seed=3, scale=0.1)
    gamma, beta = (rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1)) if ln else (None, None)
    fill = rnd(D, seed=7)
    R = fill.view(1, 1, D).expand(B, K - 1, D).contiguous() if broadcast_fill else rnd(B, K - 1, D, seed=6)
    return ConvInputs(B, T, D, K, z, w_kc, bias, gamma, beta, R, fill, cl)


def causal_conv_ref(seq, w_kc, bias, gamma, beta, eps=CONV_EPS, dtype=torch.float64):
    """seq [K - 1 + N][D] = the K - 1 frames left of the utterance, then its N frames -> [N][D]:
    y[t] = bias + sum_k w[k] seq[t + k], LayerNorm over D (gamma None: none), SiLU."""
    K = w_kc.shape[0]
    y = (seq.to(dtype).unfold(0, K, 1) * w_kc.to(dtype).t().unsqueeze(0)).sum(-1) + bias.to(dtype)
    if gamma is not None:
        mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
        y = (y - mu) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)
    return y * torch.sigmoid(y)


def conv_stream_ref(d, dtype=torch.float64):
    """Per utterance the reference over [R | z_0[:len_0] | z_1[:len_1] | ...]: a list over b of (rows [N_b][D], and the chunk
    and frame each row belongs to as a list of (n, t))."""
    res = []
    for b in range(d.B):
        parts, where = [d.R[b]], []
        for n in range(d.z.shape[0]):
            nl = int(d.chunk_lens[n, b])
            parts.append(d.z[n, b, :nl])
            where += [(n, t) for t in range(nl)]
        res.append((causal_conv_ref(torch.cat(parts), d.w_kc, d.bias, d.gamma, d.beta, dtype=dtype), where))
    return res


def next_cache(cache_b, z_b, nl):
    """the last K - 1 frames of [cache | z[:nl]] (one utterance; nl = 0: the cache itself)"""
    return torch.cat([cache_b, z_b[:max(nl, 0)]])[-cache_b.shape[0]:]
