"""References of the packed-row and bf16-row operand forms (test-side only; numpy / torch fp64, launches nothing).

  sub_len / row_plan     the row plan of a ragged batch: the subsampled lengths in C `int` arithmetic (truncating division, as
                         oracle.encoder_ref.sub_len and the kernels have it), the clamp of a length to [0, T], row0 and pad_of
  row_plan_brute         the same plan from a loop over every (utterance, frame), for test_packed_forms_host.py
  pack / unpack          padded rows <-> packed rows through a plan
  packed_attention_ref   per utterance, stream_kernels_ref.attention_ref on that utterance's own frames
  packed_dwconv_ref      the padded conv: frames len <= t < T hold the pad row, taps outside [0, T) are zero (symmetric) or, on the
                         left of the causal form, left_fill
  double_layer_norm_ref  LN2 applied to the fp32 values LN1 stores
  bf16                   rounding through torch.bfloat16
  row_stats_ref          (sum, sum of squares) of the rows of a bf16 matrix, with the worst-case bound of an fp32 sum
"""
import numpy as np
import torch

from stream_kernels_ref import attention_ref


def _trunc_div(a, b):
    """C integer division (rounds toward zero) on numpy int64"""
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def sub_len(feat_len):
    """((l - 3) / 2 + 1 - 3) / 2 + 1 in C int arithmetic: 6 -> 1, 7 -> 1, 11 -> 2; 0 only for l <= 4"""
    l = np.asarray(feat_len, dtype=np.int64)
    l1 = _trunc_div(l - 3, 2) + 1
    return _trunc_div(l1 - 3, 2) + 1


def row_plan(lens, T, feat_len=None):
    """-> (len_out [B], row0 [B + 1], pad_of [B * T], P).  len_out: `lens`, or the subsampled feat_len, as stored (unclamped);
    utterance b owns min(max(len_out[b], 0), T) rows from row0[b]; pad_of[p] = b * T + t for p < P, -1 behind."""
    len_out = sub_len(feat_len) if feat_len is not None else np.asarray(lens, dtype=np.int64)
    live = np.clip(len_out, 0, T)
    B = len(live)
    row0 = np.concatenate([[0], np.cumsum(live)]).astype(np.int64)
    P = int(row0[B])
    pad_of = np.full(B * T, -1, dtype=np.int64)
    b_of = np.repeat(np.arange(B), live)
    pad_of[:P] = b_of * T + (np.arange(P) - row0[b_of])
    return len_out.astype(np.int32), row0.astype(np.int32), pad_of.astype(np.int32), P


def row_plan_brute(lens, T, feat_len=None):
    """the plan from a plain loop over every utterance and frame, C arithmetic spelled out with Python ints"""
    def cdiv(a, b):
        return -((-a) // b) if a < 0 else a // b
    B = len(lens) if feat_len is None else len(feat_len)
    len_out, row0, pad_of = [], [0], []
    for b in range(B):
        l = int(lens[b]) if feat_len is None else cdiv(cdiv(int(feat_len[b]) - 3, 2) + 1 - 3, 2) + 1
        len_out.append(l)
        n = 0
        for t in range(T):
            if t < l:
                pad_of.append(b * T + t)
                n += 1
        row0.append(row0[-1] + n)
    P = row0[-1]
    pad_of += [-1] * (B * T - P)
    return len_out, row0, pad_of, P


def pack(padded, pad_of, P):
    """padded [B * T][n] -> packed [P][n]"""
    idx = torch.as_tensor(np.asarray(pad_of[:P], dtype=np.int64))
    return padded[idx]


def unpack(packed, row0, B, T):
    """packed [>= P][n] -> padded [B * T][n], zeros behind every utterance's last frame"""
    out = torch.zeros(B * T, packed.shape[1], dtype=packed.dtype)
    for b in range(B):
        n = int(row0[b + 1]) - int(row0[b])
        out[b * T:b * T + n] = packed[int(row0[b]):int(row0[b]) + n]
    return out


def bf16(t):
    """round to nearest even through torch.bfloat16, back in fp64"""
    return t.float().to(torch.bfloat16).double()


def packed_attention_ref(qkv_packed, p, u, v, lens, row0, T, H, dk, chunk=0, left=-1, bf16_rows=False):
    """qkv_packed [P][3 D] -> [P][D] fp64: utterance b alone, B = 1 and T = its own length (the chunk windows are cut at T in the
    kernel and at the length here: the same keys, since a key is < len).  bf16_rows: the bf16 core's reference (qkv already
    bf16 values; p, q + u and q + v rounded to bf16 as test_relpos_attention_bf16 has it)."""
    D = H * dk
    P = int(row0[-1])
    out = torch.zeros(P, D, dtype=torch.float64)
    for b in range(len(lens)):
        n = int(row0[b + 1]) - int(row0[b])
        if n == 0:
            continue
        rows = qkv_packed[int(row0[b]):int(row0[b]) + n]
        pp = bf16(p[:n]) if bf16_rows else p[:n]
        out[int(row0[b]):int(row0[b]) + n] = attention_ref(rows.reshape(1, n, 3 * D), pp, u, v, torch.tensor([n]), 1, n, H, dk, chunk, left,
                                                           round_q16=bf16_rows)
    return out


def packed_dwconv_ref(z_packed, pad_row, w_kc, bias, gamma, beta, eps, lens, row0, T, left_fill=None):
    """z_packed [P][D], pad_row [D] -> [P][D] fp64: depthwise conv + LayerNorm (gamma None: none) + SiLU of utterance b on the
    padded frames [z_b | pad_row ...] of length T.  Symmetric (left_fill None): pad (K - 1) / 2 zeros on both sides; causal:
    K - 1 frames of left_fill on the left, no taps to the right."""
    K, D = w_kc.shape
    w = w_kc.double()
    P = int(row0[-1])
    out = torch.zeros(P, D, dtype=torch.float64)
    for b in range(len(lens)):
        n = int(row0[b + 1]) - int(row0[b])
        if n == 0:
            continue
        frames = pad_row.double().view(1, D).repeat(T, 1)
        frames[:n] = z_packed[int(row0[b]):int(row0[b]) + n].double()
        if left_fill is None:
            half = (K - 1) // 2
            seq = torch.cat([torch.zeros(half, D, dtype=torch.float64), frames, torch.zeros(half, D, dtype=torch.float64)])
        else:
            seq = torch.cat([left_fill.double().view(1, D).repeat(K - 1, 1), frames])
        y = (seq.unfold(0, K, 1) * w.t().unsqueeze(0)).sum(-1) + bias.double()           # [T][D]
        if gamma is not None:
            mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
            y = (y - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()
        out[int(row0[b]):int(row0[b]) + n] = (y * torch.sigmoid(y))[:n]
    return out


def layer_norm_ref(x, gamma, beta, eps):
    x = x.double()
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def double_layer_norm_ref(y_fp32, gamma2, beta2, eps2):
    """LN2 of the fp32 values the first LayerNorm stored (y_fp32: those values, as read back)"""
    return layer_norm_ref(y_fp32, gamma2, beta2, eps2)


def row_stats_ref(xb):
    """bf16 matrix [rows][D] -> (sum [rows], sum of squares [rows], bound on sum, bound on sum of squares), fp64.  An fp32 sum of
    D terms in any order is off by at most (D - 1) u sum|term| (u = 2^-24) to first order: D * 2^-24 * sum|term| covers it, the
    fp32 rounding of every square included."""
    f = xb.float().double()
    s1, s2 = f.sum(-1), (f * f).sum(-1)
    D = f.shape[-1]
    return s1, s2, D * 2.0 ** -24 * f.abs().sum(-1), D * 2.0 ** -24 * s2
