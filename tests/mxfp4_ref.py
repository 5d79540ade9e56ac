"""The MXFP4 storage format of the expert weights, restated in float64 numpy from its written definition (not from
m3asr/plan.py, which the tests compare against this):

  * blocks: 32 consecutive elements along the GEMM's K;
  * scale byte: s = clamp(floor(log2(amax)) - 2, -64, 64) + 127, an e8m0 code; an all-zero block stores 127; a block too small
    for the clamp gets all-zero codes (it simply rounds to zero);
  * elements: w / 2^(s - 127) rounded to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating at +-6,
    the sign in bit 3 of the code (a zero carries none);
  * packing: two codes per byte, the even-k element in the low nibble.
"""
import math

import numpy as np

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
BLOCK = 32


def _code(a):
    """magnitude a >= 0 (already divided by the block scale) -> e2m1 code 0..7: nearest grid value, a tie to the even code"""
    if a >= GRID[-1]:
        return 7
    best, best_d = 0, None
    for c, g in enumerate(GRID):
        d = abs(a - g)
        if best_d is None or d < best_d or (d == best_d and c % 2 == 0):
            best, best_d = c, d
    return best


def quantize_block(v):
    """32 float64 values -> (32 codes, scale byte)"""
    assert len(v) == BLOCK
    amax = max(abs(float(t)) for t in v)
    if amax == 0.0:
        return [0] * BLOCK, 127
    m, ex = math.frexp(amax)                      # amax = m 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = min(max(ex - 1 - 2, -64), 64)
    codes = []
    for t in v:
        c = _code(math.ldexp(abs(float(t)), -e))
        codes.append(c | (8 if (t < 0 and c != 0) else 0))
    return codes, e + 127


def quantize(w):
    """w [..., K] (K % 32 == 0, blocks along the last axis) -> (bytes [..., K/2] uint8, scales [..., K/32] uint8)"""
    w = np.asarray(w, dtype=np.float64)
    K = w.shape[-1]
    assert K % BLOCK == 0
    flat = w.reshape(-1, K)
    q = np.zeros((flat.shape[0], K // 2), dtype=np.uint8)
    s = np.zeros((flat.shape[0], K // BLOCK), dtype=np.uint8)
    for r in range(flat.shape[0]):
        for b in range(K // BLOCK):
            codes, sc = quantize_block(flat[r, BLOCK * b:BLOCK * (b + 1)])
            s[r, b] = sc
            for i in range(BLOCK // 2):
                q[r, (BLOCK // 2) * b + i] = codes[2 * i] | (codes[2 * i + 1] << 4)
    return q.reshape(w.shape[:-1] + (K // 2,)), s.reshape(w.shape[:-1] + (K // BLOCK,))


def decode(q, s):
    """bytes [..., K/2], scales [..., K/32] -> float64 [..., K]"""
    q, s = np.asarray(q, dtype=np.uint8), np.asarray(s, dtype=np.uint8)
    codes = np.stack([q & 15, q >> 4], axis=-1).reshape(q.shape[:-1] + (q.shape[-1] * 2,)).astype(np.int64)
    val = GRID[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    scale = np.ldexp(1.0, s.astype(np.int64) - 127)
    return val * np.repeat(scale, BLOCK, axis=-1)
