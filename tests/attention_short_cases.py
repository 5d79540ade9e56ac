"""Cases of the fp32 attention core at short T' (test-side helper shared by tests/test_attention_short_gpu.py and
tools/record_attention_golden.py, which records what a build computes for them).

Every case is a dict {kind, id, ...}; run_case(case) launches it on guarded, row-strided operands (tests/guarded.py: NaN around
every input, a pattern around every output), checks the guards, and returns a list of Result(name, got, want, rows):
  got   the output as a dense CPU tensor (fp32, or bf16 for the rounded copy) -- what is hashed, bit for bit
  want  the float64 reference (None where `got` is only compared with another output)
  rows  the rows compared with the reference (None: all)
Inputs are torch.randn from seeded CPU generators, so a case is the same data on every machine.

  plain   ops.relpos_attention, lengths full and ragged, no chunk mask
  chunk   the static chunk mask (chunk 16, left -1 / 0 / 1): rows whose first key tiles are invisible
  packed  ops.relpos_attention_packed with a row0 plan, unowned rows poisoned with NaN, and the bf16 copy of the output
  dual    ops.relpos_attention_pair on two problems of unequal T' (50 and 33), both orders
"""
import hashlib
from collections import namedtuple

import numpy as np
import torch

import guarded as G
import packed_ref as R
from m3asr import ops
from stream_kernels_ref import attention_ref

Result = namedtuple("Result", "name got want rows")

T_ALL = [1, 15, 16, 17, 33, 48, 49, 50, 63, 64, 65, 80]          # 64 / 65: one key tile per wave / the loop's second trip
DK_ALL = [16, 32, 64, 128]
BH_ALL = [(1, 8), (2, 4), (1, 2), (3, 1)]                        # H B a multiple of 8 (XCD map on) and not
TOL = 3e-5                                                       # test_relpos_attention_strided's bound for T' < 130


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.cuda().contiguous()


def lens_of(B, T):
    """full, and ragged: a length that leaves waves 2 and 3 without a key (17), a one-frame and an empty utterance"""
    ragged = {1: [17 if T > 17 else T // 2], 2: [min(T, 17), 0], 3: [T, 1, 0]}[B]
    return {"full": [T] * B, "ragged": ragged}


def all_cases():
    cases = []
    for T in T_ALL:
        for dk in DK_ALL:
            for B, H in BH_ALL:
                cases.append(dict(kind="plain", id="plain-T%d-dk%d-B%dH%d" % (T, dk, B, H), T=T, dk=dk, B=B, H=H))
    for T in (33, 50):
        for dk in DK_ALL:
            for B, H in ((1, 8), (3, 1)):
                for left in (-1, 0, 1):
                    cases.append(dict(kind="chunk", id="chunk16-left%d-T%d-dk%d-B%dH%d" % (left, T, dk, B, H), T=T, dk=dk, B=B, H=H, left=left))
    for T in (33, 50, 65):
        for dk in DK_ALL:
            for chunk, left in ((0, -1), (16, 1)):
                cases.append(dict(kind="packed", id="packed-T%d-dk%d-chunk%d" % (T, dk, chunk), T=T, dk=dk, chunk=chunk, left=left))
    for dk0, dk1 in ((128, 64), (64, 128), (64, 64), (128, 128)):
        cases.append(dict(kind="dual", id="dual-dk%d-dk%d" % (dk0, dk1), dk0=dk0, dk1=dk1))
    return cases


def _operands(B, T, H, dk, seed):
    D = H * dk
    return (rnd(B * T, 3 * D, seed=seed + 1), rnd(T, D, seed=seed + 2), rnd(H, dk, seed=seed + 3, scale=0.3),
            rnd(H, dk, seed=seed + 4, scale=0.3))


def _padded(tag, B, T, H, dk, lens, chunk, left, seed):
    """one padded launch on strided, guarded views -> Result (every row is written; rows behind an utterance's last frame see
    the keys < len, an empty utterance gives zero rows -- the reference has both)"""
    D = H * dk
    qkv, p, u, v = _operands(B, T, H, dk, seed)
    L = torch.tensor(lens, dtype=torch.int32)
    gq, gp, go = G.strided_in(qkv, ld=3 * D + 4), G.strided_in(p, ld=D + 4), G.strided_out(B * T, D, ld=D + 4)
    ops.relpos_attention(gq.view, gp.view, dev(u), dev(v), dev(L), B, T, H, dk, chunk=chunk, left_chunks=left, out=go.view)
    torch.cuda.synchronize()
    go.check(tag)
    assert not bool(go.untouched().any()), tag + ": a row is not written"
    got = G.dense(go.view).cpu()
    for b in range(B):
        if lens[b] == 0:
            assert not bool(got[b * T:(b + 1) * T].any()), tag + ": an empty utterance's rows are not zero"
    return Result(tag, got, attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left), None)


def _run_plain(c):
    return [_padded("%s/%s" % (c["id"], name), c["B"], c["T"], c["H"], c["dk"], lens, 0, -1, 10)
            for name, lens in lens_of(c["B"], c["T"]).items()]


def _run_chunk(c):
    return [_padded("%s/%s" % (c["id"], name), c["B"], c["T"], c["H"], c["dk"], lens, 16, c["left"], 20)
            for name, lens in lens_of(c["B"], c["T"]).items()]


def _run_packed(c):
    T, dk, chunk, left, H = c["T"], c["dk"], c["chunk"], c["left"], 2
    lens = [16, 1, 0, 17, 15, T]
    B, D = len(lens), H * dk
    qkv, p, u, v = _operands(B, T, H, dk, 30)
    len_out, row0, pad_of, P = R.row_plan(lens, T)
    L, row0_d = dev(torch.as_tensor(len_out)), dev(torch.as_tensor(row0))
    idx = torch.as_tensor(pad_of[:P].astype(np.int64))
    packed = qkv[idx]
    gp = G.strided_in(p)
    args = (gp.view, dev(u), dev(v), L, B, T, H, dk)
    out_pad = ops.relpos_attention(dev(qkv), *args, chunk=chunk, left_chunks=left)
    gq, go, gb = G.strided_in(packed), G.strided_out(P, D), G.strided_out(P, D, torch.bfloat16)
    ops.relpos_attention_packed(gq.view, *args, out=go.view, row0=row0_d, chunk=chunk, left_chunks=left)
    ops.relpos_attention_packed(gq.view, *args, out=gb.view, row0=row0_d, chunk=chunk, left_chunks=left)
    torch.cuda.synchronize()
    tag = c["id"]
    go.check(tag)
    gb.check(tag + " out_bf16")
    assert not bool(go.untouched().any()) and not bool(gb.untouched().any()), tag + ": a live row is not written"
    got = G.dense(go.view)
    assert G.same_bits(got, out_pad[idx.cuda()]), tag + ": packed rows differ from the padded call"
    assert G.same_bits(G.dense(gb.view), got.to(torch.bfloat16)), tag + ": the bf16 output is not the rounded fp32 output"
    r0 = row0.tolist()
    for b in range(B):                                           # NaN in every row the utterance does not own
        if r0[b + 1] == r0[b]:
            continue
        alone = torch.full_like(packed, float("nan"))
        alone[r0[b]:r0[b + 1]] = packed[r0[b]:r0[b + 1]]
        gn = G.strided_out(P, D)
        ops.relpos_attention_packed(G.strided_in(alone).view, *args, out=gn.view, row0=row0_d, chunk=chunk, left_chunks=left)
        torch.cuda.synchronize()
        gn.check(tag + " (NaN neighbours)")
        assert G.same_bits(G.dense(gn.view[r0[b]:r0[b + 1]]), got[r0[b]:r0[b + 1]]), tag + ": utterance %d read a row it does not own" % b
    want = R.packed_attention_ref(packed, p, u, v, lens, row0, T, H, dk, chunk, left)
    return [Result(tag + "/f32", got.cpu(), want, None), Result(tag + "/bf16", G.dense(gb.view).cpu(), None, None)]


def _run_dual(c):
    """problem a: the embed encoder's shape (H = 4) at T' = 50, chunk mask; problem b: B = 2, H = 4 (XCD map on) at T' = 33, ragged"""
    probs = [dict(B=1, T=50, H=4, dk=c["dk0"], lens=[50], chunk=16, left=1, seed=40),
             dict(B=2, T=33, H=4, dk=c["dk1"], lens=[33, 17], chunk=0, left=-1, seed=50)]
    ins, single = [], []
    for q in probs:
        B, T, H, dk = q["B"], q["T"], q["H"], q["dk"]
        D = H * dk
        qkv, p, u, v = _operands(B, T, H, dk, q["seed"])
        L = torch.tensor(q["lens"], dtype=torch.int32)
        gq, gp = G.strided_in(qkv), G.strided_in(p, ld=2 * D)
        kw = dict(qkv=gq.view, p=gp.view, pos_u=dev(u), pos_v=dev(v), lens=dev(L), B=B, T=T, H=H, dk=dk, chunk=q["chunk"], left_chunks=q["left"])
        ins.append((kw, (B * T, D), attention_ref(qkv, p, u, v, L, B, T, H, dk, q["chunk"], q["left"])))
        go = G.strided_out(B * T, D)
        ops.relpos_attention(out=go.view, **kw)
        torch.cuda.synchronize()
        go.check(c["id"] + " single")
        single.append(G.dense(go.view))
    res = []
    for order in ((0, 1), (1, 0)):
        outs = [G.strided_out(*ins[i][1]) for i in order]
        ops.relpos_attention_pair(*[dict(out=o.view, **ins[i][0]) for i, o in zip(order, outs)])
        torch.cuda.synchronize()
        for i, o in zip(order, outs):
            tag = "%s/order%d%d/problem%d" % (c["id"], order[0], order[1], i)
            o.check(tag)
            assert not bool(o.untouched().any()), tag + ": a row is not written"
            assert G.same_bits(G.dense(o.view), single[i]), tag + ": the paired launch differs from the single launch"
            res.append(Result(tag, G.dense(o.view).cpu(), ins[i][2], None))
    return res


_RUN = {"plain": _run_plain, "chunk": _run_chunk, "packed": _run_packed, "dual": _run_dual}


def run_case(c):
    return _RUN[c["kind"]](c)


def digest(t):
    """sha256 over the tensor's shape, dtype and bytes"""
    t = t.contiguous()
    raw = t.view(torch.int16).numpy().tobytes() if t.dtype == torch.bfloat16 else t.numpy().tobytes()
    return hashlib.sha256(("%s %s " % (tuple(t.shape), t.dtype)).encode() + raw).hexdigest()
