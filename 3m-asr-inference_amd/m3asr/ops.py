"""Torch-tensor front end of the C ABI: device memory and streams come from PyTorch-ROCm, every
computation is a libm3asr_hip.so call (include/m3asr.h).  No op here has a torch fallback."""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "m3asr ops need contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def _f32(t):
    assert t is None or t.dtype == torch.float32, "fp32 tensor expected"
    return _p(t)


def _i32(t):
    assert t is None or t.dtype == torch.int32, "int32 tensor expected"
    return _p(t)


def _rows(t, dtype=torch.float32):
    """(pointer, row stride in elements) of a 2-D operand the ABI takes with a leading dimension: any row-strided view with
    unit column stride (a column slice of a wider buffer, q|k|v, a GLU half); the launcher checks the stride itself."""
    assert t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype == dtype, "row-strided 2-D %s device tensor expected" % dtype
    return C.c_void_p(t.data_ptr()), t.stride(0)


# ---------------------------------------------------------------------------------------- MoE
def moe_scatter_mapping(gate_idx, num_expert, want_pos=True):
    lib = _lib.load()
    g = gate_idx.reshape(-1)
    S = g.numel()
    mapping = torch.empty(S, dtype=torch.int32, device=g.device)
    acc = torch.empty(num_expert + 1, dtype=torch.int32, device=g.device)
    pos = torch.empty(S, dtype=torch.int32, device=g.device) if want_pos else None
    check(lib.m3_moe_scatter_mapping(_i32(g), S, num_expert, _p(mapping), _p(acc), _p(pos), _stream()),
          "m3_moe_scatter_mapping")
    return mapping, acc, pos


def moe_local_scatter(x, mapping, n_rows):
    lib = _lib.load()
    S, row_bytes = x.shape[0], x[0].numel() * x.element_size()
    out = torch.zeros((n_rows,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    check(lib.m3_moe_local_scatter(_p(x), _i32(mapping), S, row_bytes, _p(out), _stream()), "m3_moe_local_scatter")
    return out


def moe_local_scatter_into(x, mapping, out):
    """out[mapping[s]] = x[s] for mapping[s] >= 0, into a caller-owned buffer (rows of out not hit keep their content)."""
    lib = _lib.load()
    S, row_bytes = x.shape[0], x[0].numel() * x.element_size()
    check(lib.m3_moe_local_scatter(_p(x), _i32(mapping), S, row_bytes, _p(out), _stream()), "m3_moe_local_scatter")
    return out


def ep_send_map(gate_idx, mapping, acc, world, e_loc, capacity, map_send, wire):
    """Expert-parallel send plan on the device (m3_ep_send_map): fills map_send[S] and the header rows of `wire`
    [world, 1 + capacity, D]."""
    lib = _lib.load()
    S = gate_idx.numel()
    row_bytes = wire.shape[-1] * wire.element_size()
    check(lib.m3_ep_send_map(_i32(gate_idx.reshape(-1)), _i32(mapping), _i32(acc), S, world, e_loc, capacity, _p(map_send),
                             _p(wire), row_bytes, _stream()), "m3_ep_send_map")
    return map_send


def ep_recv_gate(wire, world, e_loc, capacity, gate_recv):
    """Local expert id of every received wire row (m3_ep_recv_gate)."""
    lib = _lib.load()
    row_bytes = wire.shape[-1] * wire.element_size()
    check(lib.m3_ep_recv_gate(_p(wire), world, e_loc, capacity, row_bytes, _p(gate_recv), _stream()), "m3_ep_recv_gate")
    return gate_recv


def moe_local_gather(buf, mapping):
    lib = _lib.load()
    S = mapping.numel()
    row_bytes = buf[0].numel() * buf.element_size()
    out = torch.empty((S,) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
    check(lib.m3_moe_local_gather(_p(buf), _i32(mapping), S, row_bytes, _p(out), _stream()), "m3_moe_local_gather")
    return out


def moe_expert_workspace_size(S, E, D, F):
    return _lib.load().m3_moe_expert_workspace_size(S, E, D, F)


def quantize_rows_e4m3(x):
    """x (S, 512) f32 -> (xq (S, 512) uint8 holding OCP e4m3, scale (S,) f32): scale = amax / 448 per row, round to nearest even,
    saturating -- what the fused fp8 expert kernel does to its input rows (m3_quantize_rows_e4m3)."""
    lib = _lib.load()
    S, D = x.shape
    xp, ldx = _rows(x)
    xq = torch.empty(S, D, dtype=torch.uint8, device=x.device)
    scale = torch.empty(S, dtype=torch.float32, device=x.device)
    check(lib.m3_quantize_rows_e4m3(xp, ldx, S, D, _p(xq), _p(scale), _stream()), "m3_quantize_rows_e4m3")
    return xq, scale


def moe_expert_ffn(x, gate_idx, w1, b1, w2, b2, gate_value=None, resid=None, alpha=1.0, ln=None, workspace=None,
                   w1_scale=None, w2_scale=None, out=None, h_scale=None, xq=None, xq_scale=None):
    """FMoEExpert: x (S,D) f32, gate_idx (S,) i32 -> y (S,D).  Optional fused epilogue (gate, residual, LayerNorm).
    The expert weights pick the kernel family: fp32; bf16 (bf16 MFMA, fp32 accumulate); e4m3 with per-row scales
    w1_scale [E,F] / w2_scale [E,D]; uint8 MXFP4 code pairs with uint8 block scales (decoded to bf16 at the MFMA input,
    m3_moe_expert_ffn_mxfp4) (fp8: dequantised to bf16 at the MFMA input; with h_scale: fp8 arithmetic, activations
    quantised too -- m3_moe_expert_ffn_fp8a8; xq / xq_scale: the rows already quantised by quantize_rows_e4m3, read instead
    of x where the fused kernel applies -- m3_moe_expert_ffn_fp8a8_xq).  Biases are fp32 in every mode.
    fp32 w1 (E, F/16, D/16, 4, 16, 4) with w2 (E, F/slice, D/16, slice/16, 4, 16, 4): fragment order (plan.pack_wfrag of w1 and
    of the slice-major w2), m3_moe_expert_ffn_wfrag."""
    lib = _lib.load()
    assert w1.dtype == w2.dtype and w1.is_contiguous() and w2.is_contiguous()
    S, D = x.shape
    wfrag = w1.dim() == 6
    assert not wfrag or (w1.dtype == torch.float32 and w2.dim() == 7)
    E, F = w1.shape[0], w1.shape[1] * (16 if wfrag else 1)
    if workspace is None:
        workspace = torch.empty(max(moe_expert_workspace_size(S, E, D, F), 1), dtype=torch.uint8, device=x.device)
    y = out if out is not None else torch.empty_like(x)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    gate = _f32(gate_value.reshape(-1) if gate_value is not None else None)
    tail = (S, E, D, F, gate, _f32(resid), float(alpha), _f32(g), _f32(b), float(eps), _p(y), _p(workspace),
            workspace.numel(), _stream())
    xi, gi = _f32(x), _i32(gate_idx.reshape(-1))
    if w1.dtype == torch.float8_e4m3fn and h_scale is not None:
        # fp8 arithmetic: activations quantised too (rows: per-row dynamic scale; H: the static scale h_scale)
        assert w1_scale is not None and w2_scale is not None, "fp8 expert weights need their per-row scales"
        if xq is not None:
            assert xq.dtype in (torch.uint8, torch.float8_e4m3fn) and xq.is_contiguous() and xq.shape == x.shape and xq_scale is not None
            check(lib.m3_moe_expert_ffn_fp8a8_xq(xi, _p(xq), _f32(xq_scale), gi, _p(w1), _f32(w1_scale), _f32(b1), _p(w2),
                                                 _f32(w2_scale), _f32(b2), float(h_scale), *tail), "m3_moe_expert_ffn_fp8a8_xq")
            return y
        check(lib.m3_moe_expert_ffn_fp8a8(xi, gi, _p(w1), _f32(w1_scale), _f32(b1), _p(w2), _f32(w2_scale), _f32(b2),
                                          float(h_scale), *tail), "m3_moe_expert_ffn_fp8a8")
    elif w1.dtype == torch.float8_e4m3fn:
        assert w1_scale is not None and w2_scale is not None, "fp8 expert weights need their per-row scales"
        check(lib.m3_moe_expert_ffn_fp8(xi, gi, _p(w1), _f32(w1_scale), _f32(b1), _p(w2), _f32(w2_scale), _f32(b2), *tail),
              "m3_moe_expert_ffn_fp8")
    elif w1.dtype == torch.uint8:
        # MXFP4 (plan.quantize_mxfp4 along K): w1 [E,F,D/2] + w1_scale [E,F,D/32], w2 [E,D,F/2] + w2_scale [E,D,F/32], all uint8
        assert w1_scale is not None and w2_scale is not None and w1_scale.dtype == torch.uint8 and w2_scale.dtype == torch.uint8, \
            "mxfp4 expert weights need their uint8 block scales"
        assert w1.shape[2] * 2 == D and tuple(w2.shape) == (E, D, F // 2), "mxfp4 expert weights: two codes per byte along K"
        assert tuple(w1_scale.shape) == (E, F, D // 32) and tuple(w2_scale.shape) == (E, D, F // 32)
        assert w1_scale.is_contiguous() and w2_scale.is_contiguous()
        check(lib.m3_moe_expert_ffn_mxfp4(xi, gi, _p(w1), _p(w1_scale), _f32(b1), _p(w2), _p(w2_scale), _f32(b2), *tail),
              "m3_moe_expert_ffn_mxfp4")
    elif w1.dtype == torch.bfloat16:
        check(lib.m3_moe_expert_ffn_bf16(xi, gi, _p(w1), _f32(b1), _p(w2), _f32(b2), *tail), "m3_moe_expert_ffn_bf16")
    elif wfrag:
        check(lib.m3_moe_expert_ffn_wfrag(xi, gi, _f32(w1), _f32(b1), _f32(w2), _f32(b2), *tail), "m3_moe_expert_ffn_wfrag")
    else:
        check(lib.m3_moe_expert_ffn(xi, gi, _f32(w1), _f32(b1), _f32(w2), _f32(b2), *tail), "m3_moe_expert_ffn")
    return y


def moe_combine(rows, mapping, gate_value=None, resid=None, alpha=1.0, ln=None, out=None, out_bf16=None):
    """out[s] = LN(resid[s] + alpha * gate[s] * rows[mapping[s]]); rows are in scattered (expert-sorted) order.
    out_bf16 (optional, (S, D) bf16): also receives the result rounded to bf16 (the engine's "xb" copy)."""
    lib = _lib.load()
    S, D = mapping.numel(), rows.shape[-1]
    y = out if out is not None else torch.empty(S, D, dtype=torch.float32, device=rows.device)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    if out_bf16 is not None:
        assert out_bf16.dtype == torch.bfloat16 and out_bf16.numel() >= S * D and out_bf16.is_contiguous()
        check(lib.m3_moe_combine_bf16(_f32(rows), _i32(mapping), _f32(gate_value.reshape(-1) if gate_value is not None else None),
                                      _f32(resid), float(alpha), _f32(g), _f32(b), float(eps), _p(y), _p(out_bf16), S, D, _stream()),
              "m3_moe_combine_bf16")
        return y
    check(lib.m3_moe_combine(_f32(rows), _i32(mapping), _f32(gate_value.reshape(-1) if gate_value is not None else None),
                             _f32(resid), float(alpha), _f32(g), _f32(b), float(eps), _p(y), S, D, _stream()),
          "m3_moe_combine")
    return y


def moe_router(embed, x, w, ln, bias=None, want_xn=True, out=None, xn_out=None, live_rows=None):
    """logits (S, E) = cat([embed, LayerNorm(x)]) @ w^T (+ bias), xn = LayerNorm(x); w (E, De + D) fp32, ln = (gamma, beta, eps).
    embed / x and the optional result buffers out (S, E) / xn_out (S, D) may be row-strided views.
    live_rows: one int32 on the device, the count of live rows of a packed ragged batch (m3_moe_router_live_rows)."""
    lib = _lib.load()
    S, De = embed.shape
    D = x.shape[1]
    E = w.shape[0]
    assert w.shape[1] == De + D and w.is_contiguous()
    logits = out if out is not None else torch.empty(S, E, dtype=torch.float32, device=x.device)
    xn = xn_out if xn_out is not None else (torch.empty(S, D, dtype=torch.float32, device=x.device) if want_xn else None)
    assert tuple(logits.shape) == (S, E) and (xn is None or tuple(xn.shape) == (S, D))
    (ep, lde), (xp, ldx), (lp, ldl) = _rows(embed), _rows(x), _rows(logits)
    xnp, ldxn = _rows(xn) if xn is not None else (None, D)
    if live_rows is not None:
        check(lib.m3_moe_router_live_rows(ep, lde, De, xp, ldx, D, _f32(w), _f32(bias), _f32(ln[0]), _f32(ln[1]), float(ln[2]),
                                          xnp, ldxn, lp, ldl, S, E, _i32(live_rows), _stream()), "m3_moe_router_live_rows")
        return logits, xn
    check(lib.m3_moe_router(ep, lde, De, xp, ldx, D, _f32(w), _f32(bias), _f32(ln[0]), _f32(ln[1]), float(ln[2]),
                            xnp, ldxn, lp, ldl, S, E, _stream()), "m3_moe_router")
    return logits, xn


def softmax_top1(logits, lens=None, rows_per_batch=0):
    lib = _lib.load()
    E = logits.shape[-1]
    l2 = logits if logits.dim() == 2 else logits.reshape(-1, E)      # a 2-D operand may be a row-strided view
    S = l2.shape[0]
    idx = torch.empty(S, dtype=torch.int32, device=logits.device)
    val = torch.empty(S, dtype=torch.float32, device=logits.device)
    lp, ld = _rows(l2)
    check(lib.m3_softmax_top1(lp, ld, _i32(lens), rows_per_batch, S, E, _p(idx), _p(val), _stream()),
          "m3_softmax_top1")
    return val, idx


def _route_taps(S, E, device, taps):
    """(gate_idx, gate_value, mapping, acc_histogram, pos) of the routing entry points: the caller's buffers or fresh ones"""
    if taps is None:
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=device)   # noqa: E731
        taps = (i32(S), torch.empty(S, dtype=torch.float32, device=device), i32(S), i32(E + 1), i32(S))
    gi, gv, mp, acc, pos = taps
    assert gi.numel() == S and gv.numel() == S and mp.numel() == S and acc.numel() == E + 1 and (pos is None or pos.numel() == S)
    return taps, (_i32(gi), _f32(gv), _i32(mp), _i32(acc), _i32(pos))


def moe_gate_index(logits, row_len=None, rows_per_batch=0, taps=None):
    """SoftmaxTopK + ScatterMapping in one launch (m3_moe_gate_index): logits (S, E) dense -> (gate_idx, gate_value, mapping,
    acc_histogram (E + 1), pos); frames t >= row_len[b] of rows_per_batch-frame utterances are dropped."""
    lib = _lib.load()
    S, E = logits.shape
    taps, ptrs = _route_taps(S, E, logits.device, taps)
    check(lib.m3_moe_gate_index(_f32(logits), _i32(row_len), rows_per_batch, S, E, *ptrs, _stream()), "m3_moe_gate_index")
    return taps


def moe_route(x, wx, wsum, bias=None, eall=None, ln_eps=1e-12, row_len=None, rows_per_batch=0, taps=None):
    """Router x half with the LayerNorm folded into wx (E, D) / wsum (E) / bias (fold_layernorm of m3asr/plan.py), + the embed
    half eall (S, E), + SoftmaxTopK + ScatterMapping in one launch (m3_moe_route).  x / eall may be row-strided views.
    -> (gate_idx, gate_value, mapping, acc_histogram, pos)"""
    lib = _lib.load()
    S, D = x.shape
    E = wx.shape[0]
    assert tuple(wx.shape) == (E, D) and wsum.numel() == E and (bias is None or bias.numel() == E)
    xp, ldx = _rows(x)
    ep, lde = _rows(eall) if eall is not None else (None, E)
    assert eall is None or tuple(eall.shape) == (S, E)
    taps, ptrs = _route_taps(S, E, x.device, taps)
    check(lib.m3_moe_route(xp, ldx, D, _f32(wx), _f32(wsum), _f32(bias), ep, lde, float(ln_eps), _i32(row_len), rows_per_batch,
                           S, E, *ptrs, _stream()), "m3_moe_route")
    return taps


def moe_route_expert_workspace_size(S, E, D, F):
    return _lib.load().m3_moe_route_expert_workspace_size(S, E, D, F)


def moe_route_expert_ffn(x, logits, w1, b1, w2, b2, row_len=None, rows_per_batch=0, w2_sliced=False, norm=None,
                         use_gate_value=True, resid=None, alpha=1.0, ln=None, workspace=None, out=None, taps=None):
    """The self-routing expert launch + its combine (m3_moe_route_expert_ffn): router logits (S, E) -> top-1 routing, grouped
    fp32 expert FFN, y = LN(resid + alpha * gate * ffn(x)) in two launches, S <= 256.  x (S, D) may be a row-strided view;
    norm = (gamma, beta, eps): LayerNorm applied to x inside the expert kernel.  w2 (E, D, F); w2_sliced: the kernel reads
    the slice-major layout of m3asr/plan.py (w2 already 4-D: taken as repacked).  A 6-D w1 with a 7-D w2: both in fragment order
    (plan.pack_wfrag of w1 and of the slice-major w2; w2_sliced = 2 at the ABI).  -> (y, (gate_idx, gate_value, mapping,
    acc_histogram, pos))"""
    lib = _lib.load()
    S, D = x.shape
    wfrag = w1.dim() == 6
    assert not wfrag or (w2.dim() == 7 and w2.is_contiguous())
    E, F = w1.shape[0], w1.shape[1] * (16 if wfrag else 1)
    assert tuple(logits.shape) == (S, E) and w1.is_contiguous()
    if w2_sliced and w2.dim() == 3:
        from .plan import slice_major_w2
        w2 = slice_major_w2(w2)
    if workspace is None:
        workspace = torch.empty(max(moe_route_expert_workspace_size(S, E, D, F), 1), dtype=torch.uint8, device=x.device)
    y = out if out is not None else torch.empty(S, D, dtype=torch.float32, device=x.device)
    xp, ldx = _rows(x)
    ng, nb, neps = norm if norm is not None else (None, None, 0.0)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    taps, ptrs = _route_taps(S, E, x.device, taps)
    check(lib.m3_moe_route_expert_ffn(xp, ldx, _f32(logits), _i32(row_len), rows_per_batch, _f32(w1), _f32(b1), _f32(w2),
                                      2 if wfrag else (1 if w2_sliced else 0), _f32(b2), S, E, D, F, _f32(ng), _f32(nb), float(neps),
                                      1 if use_gate_value else 0, _f32(resid), float(alpha), _f32(g), _f32(b), float(eps),
                                      *ptrs, _p(y), _p(workspace), workspace.numel() * workspace.element_size(), _stream()),
          "m3_moe_route_expert_ffn")
    return y, taps


# ---------------------------------------------------------------------------------------- dense
def linear(a, w, bias=None, act=_lib.ACT_NONE, a2=None, ln=None, lens=None, rows_per_batch=0, mask_in=False,
           mask_out=False, alpha=1.0, resid=None, out=None, ln_folded=None, split_k=False, out_dtype=torch.float32,
           copy_bf16=None, copy_stats=None, ln_stats=None, workspace=None, live_rows=None, _kernel_only=False, _desc_only=False):
    """y = resid + alpha * mask_out(act(LN(mask_in(cat[a,a2])) @ w^T + bias)); a (M,K1), w (N,K).
    ln = (gamma, beta, eps): affine LayerNorm prologue.  ln_folded = (wsum, wbeta or None, eps): w / bias already
    contain the LayerNorm affine (plan.fold_layernorm) and the kernel normalises its output.
    bf16 activation operands (bf16 weights only): `a` may be a bf16 tensor; out_dtype=torch.bfloat16 writes y as bf16;
    copy_bf16 (M, n_out) bf16 receives an extra bf16 copy of y, copy_stats (M, n_out/128, 2) f32 its per-tile row statistics;
    ln_stats (M, parts, 2): such statistics of a bf16 `a`, which the folded LayerNorm then uses.
    a, a2, y (= out), resid and copy_bf16 may be row-strided views (unit column stride); their row strides go to the ABI.
    workspace (split_k only): caller-owned uint8 scratch of at least m3_linear_workspace_size bytes.
    A 5-D w (N/16, K/16, 4, 16, 4) is taken as fragment-ordered (plan.pack_wfrag) and runs m3_linear_wfrag.
    live_rows: one int32 on the device, the count of live rows of a packed ragged batch (m3_linear_live_rows)."""
    lib = _lib.load()
    M, K1 = a.shape
    wfrag = w.dim() == 5
    if wfrag:
        assert tuple(w.shape[2:]) == (4, 16, 4) and w.dtype == torch.float32 and not split_k
        N, K = 16 * w.shape[0], 16 * w.shape[1]
    else:
        N, K = w.shape
    n_out = N // 2 if act == _lib.ACT_GLU else N
    y = out if out is not None else torch.empty(M, n_out, dtype=out_dtype, device=a.device)
    for t in (a, a2, y, resid, copy_bf16):
        assert t is None or (t.is_cuda and t.dim() == 2 and t.stride(1) == 1), "row-strided 2-D device tensor expected"
    assert tuple(y.shape) == (M, n_out) and (resid is None or tuple(resid.shape) == (M, n_out))
    d = _lib.LinearDesc()
    d.a, d.lda = a.data_ptr(), a.stride(0)
    assert a.dtype in (torch.float32, torch.bfloat16) and y.dtype in (torch.float32, torch.bfloat16)
    d.a_dtype = _lib.BF16 if a.dtype == torch.bfloat16 else _lib.F32
    d.y_dtype = _lib.BF16 if y.dtype == torch.bfloat16 else _lib.F32
    if copy_bf16 is not None:
        assert copy_bf16.dtype == torch.bfloat16 and tuple(copy_bf16.shape) == (M, n_out)
        d.y_copy_bf16, d.ld_copy = copy_bf16.data_ptr(), copy_bf16.stride(0)
    if copy_stats is not None:
        assert copy_bf16 is not None and copy_stats.dtype == torch.float32 and copy_stats.is_contiguous()
        d.y_copy_stats = copy_stats.data_ptr()
    if ln_stats is not None:
        assert ln_stats.dtype == torch.float32 and ln_stats.is_contiguous() and ln_stats.shape[0] == M
        d.ln_stats, d.ln_stat_parts = ln_stats.data_ptr(), ln_stats.shape[1]
    if a2 is not None:
        d.a2, d.lda2, d.k1 = a2.data_ptr(), a2.stride(0), K1
        assert K1 + a2.shape[1] == K
    else:
        assert K1 == K
    assert w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous()
    d.w, d.bias = w.data_ptr(), (bias.data_ptr() if bias is not None else None)
    d.weight_dtype = _lib.BF16 if w.dtype == torch.bfloat16 else _lib.F32   # bf16 weights -> bf16 MFMA, fp32 accumulate
    d.y, d.ldy = y.data_ptr(), y.stride(0)
    d.M, d.N, d.K = M, N, K
    if ln is not None:
        d.ln_gamma, d.ln_beta, d.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), float(ln[2])
    if ln_folded is not None:
        d.ln_wsum, d.ln_eps = ln_folded[0].data_ptr(), float(ln_folded[2])
        if ln_folded[1] is not None:
            d.ln_wbeta = ln_folded[1].data_ptr()
    if lens is not None:
        d.len, d.rows_per_batch = lens.data_ptr(), rows_per_batch
    d.mask_in, d.mask_out = int(mask_in), int(mask_out)
    d.act, d.alpha = act, float(alpha)
    if resid is not None:
        d.resid, d.ldr = resid.data_ptr(), resid.stride(0)
    if _desc_only:
        return d, y
    if _kernel_only:
        if live_rows is not None:
            assert not wfrag
            name = lib.m3_linear_live_rows_kernel(C.byref(d), int(bool(split_k)))
        else:
            name = lib.m3_linear_wfrag_kernel(C.byref(d)) if wfrag else lib.m3_linear_kernel(C.byref(d), int(bool(split_k)))
        return name.decode() if name else None
    if live_rows is not None:
        assert not wfrag and live_rows.numel() == 1
        need = lib.m3_linear_workspace_size(C.byref(d)) if split_k else 0
        ws = workspace if workspace is not None else (torch.empty(max(need, 1), dtype=torch.uint8, device=a.device) if split_k else None)
        check(lib.m3_linear_live_rows(C.byref(d), _i32(live_rows), _p(ws), need, _stream()), "m3_linear_live_rows")
        return y
    if wfrag:
        check(lib.m3_linear_wfrag(C.byref(d), _stream()), "m3_linear_wfrag")
        return y
    if split_k:        # deep-K / few-tile problems: split-K kernel + reduce through a scratch workspace
        need = lib.m3_linear_workspace_size(C.byref(d))
        ws = workspace if workspace is not None else torch.empty(max(need, 1), dtype=torch.uint8, device=a.device)
        assert ws.dtype == torch.uint8 and ws.numel() >= need
        check(lib.m3_linear_ws(C.byref(d), _p(ws), need, _stream()), "m3_linear_ws")
        return y
    check(lib.m3_linear(C.byref(d), _stream()), "m3_linear")
    return y


def linear_kernel(*args, **kw):
    """name of the device kernel linear(*args, **kw) would run (host-only query, m3_linear_kernel); None if it is rejected"""
    return linear(*args, _kernel_only=True, **kw)


# ---- the paired launches (include/m3asr.h "paired launches"): each problem is given as the keyword dict of its single wrapper
def _linear_desc(kw):
    kw = dict(kw)
    return linear(kw.pop("a"), kw.pop("w"), _desc_only=True, **kw)


def linear_workspace_size(**kw):
    """m3_linear_workspace_size of linear(**kw): bytes of split-K scratch, 0 where the problem is no split-K problem"""
    return _lib.load().m3_linear_workspace_size(C.byref(_linear_desc(kw)[0]))


def linear_pair(a, b):
    """linear(**a) and linear(**b) in one launch (m3_linear_pair; m3_linear_pair_wfrag when both w are fragment-ordered);
    returns (y_a, y_b)"""
    (da, ya), (db, yb) = _linear_desc(a), _linear_desc(b)
    nfrag = (a["w"].dim() == 5) + (b["w"].dim() == 5)
    assert nfrag != 1, "linear_pair: the two problems must agree on the weight layout"
    fn = "m3_linear_pair_wfrag" if nfrag else "m3_linear_pair"
    check(getattr(_lib.load(), fn)(C.byref(da), C.byref(db), _stream()), fn)
    return ya, yb


def linear_pair_kernel(a, b, with_workspace=False):
    """label of the paired kernel (host-only query, m3_linear_pair_kernel); None if the pair is refused"""
    name = _lib.load().m3_linear_pair_kernel(C.byref(_linear_desc(a)[0]), C.byref(_linear_desc(b)[0]), int(bool(with_workspace)))
    return name.decode() if name else None


def linear_ws_pair(a, ws_a, b, ws_b, which=3):
    """two split-K problems in one GEMM launch (which & 1) and one reduce launch (which & 2): m3_linear_ws_pair.  ws_a / ws_b:
    uint8 scratch of at least linear_workspace_size bytes each."""
    (da, ya), (db, yb) = _linear_desc(a), _linear_desc(b)
    check(_lib.load().m3_linear_ws_pair(C.byref(da), _p(ws_a), ws_a.numel(), C.byref(db), _p(ws_b), ws_b.numel(), int(which), _stream()),
          "m3_linear_ws_pair")
    return ya, yb


def _attention_desc(qkv, p, pos_u, pos_v, lens, B, T, H, dk, chunk=0, left_chunks=-1, out=None):
    D = H * dk
    if out is None:
        out = torch.empty(B * T, D, dtype=torch.float32, device=qkv.device)
    assert tuple(qkv.shape) == (B * T, 3 * D) and tuple(p.shape)[1] == D and p.shape[0] >= T and tuple(out.shape) == (B * T, D)
    d = _lib.AttentionDesc()
    (d.qkv, d.ldq), (d.p, d.ldp), (d.out, d.ldo) = [(q.value, ld) for q, ld in (_rows(qkv), _rows(p), _rows(out))]
    d.pos_u, d.pos_v, d.len = _f32(pos_u).value, _f32(pos_v).value, (_i32(lens).value if lens is not None else None)
    d.B, d.T, d.H, d.dk, d.scale, d.chunk, d.left_chunks = B, T, H, dk, 1.0 / math.sqrt(dk), int(chunk), int(left_chunks)
    return d, out


def relpos_attention_pair(a, b):
    """relpos_attention(**a) and relpos_attention(**b) in one launch (m3_relpos_attention_pair); returns (out_a, out_b)"""
    (da, oa), (db, ob) = _attention_desc(**a), _attention_desc(**b)
    check(_lib.load().m3_relpos_attention_pair(C.byref(da), C.byref(db), _stream()), "m3_relpos_attention_pair")
    return oa, ob


def _dwconv_desc(z, w_kc, bias, gamma, beta, eps, B, T, out=None, left_fill=None, glu=False, gate_sigmoided=False):
    K, D = w_kc.shape
    d = _lib.DwconvDesc()
    if glu:                      # z: value | gate rows, may be a row-strided view
        assert tuple(z.shape) == (B * T, 2 * D)
        zp, d.ldz = _rows(z)
        d.z = zp.value
    else:
        assert z.numel() == B * T * D
        d.z = _f32(z).value
    d.gate_sigmoided = int(bool(gate_sigmoided))
    if out is None:
        out = torch.empty(B * T, D, dtype=torch.float32, device=z.device)
    d.w_kc, d.bias, d.out = _f32(w_kc).value, _f32(bias).value, _f32(out).value
    d.gamma, d.beta = (_f32(gamma).value if gamma is not None else None), (_f32(beta).value if beta is not None else None)
    d.left_fill = _f32(left_fill).value if left_fill is not None else None
    d.eps, d.B, d.T, d.D, d.K = float(eps), B, T, D, K
    return d, out


def dwconv_ln_silu_pair(a, b):
    """two depthwise conv + LayerNorm + SiLU problems in one launch (m3_dwconv_ln_silu_pair).  Keys of a / b: z, w_kc, bias, gamma,
    beta, eps, B, T and optionally out, left_fill (causal), glu (z holds value | gate rows), gate_sigmoided."""
    (da, oa), (db, ob) = _dwconv_desc(**a), _dwconv_desc(**b)
    check(_lib.load().m3_dwconv_ln_silu_pair(C.byref(da), C.byref(db), _stream()), "m3_dwconv_ln_silu_pair")
    return oa, ob


def _conv1_desc(feat, w9c, bias, act=_lib.ACT_RELU, cmvn=None, out=None, feat_len=None, lens_out=None):
    B, T, idim = feat.shape
    Cc = w9c.shape[1]
    if out is None:
        out = torch.empty(B, (T - 3) // 2 + 1, (idim - 3) // 2 + 1, Cc, dtype=torch.float32, device=feat.device)
    d = _lib.Conv1Desc()
    d.feat, d.w9c, d.bias, d.out = _f32(feat).value, _f32(w9c).value, _f32(bias).value, _f32(out).value
    if cmvn is not None:
        d.cmvn_mean, d.cmvn_istd = _f32(cmvn[0]).value, _f32(cmvn[1]).value
    d.B, d.T, d.idim, d.C, d.act = B, T, idim, Cc, int(act)
    if feat_len is not None:
        d.feat_len, d.lens_out = _i32(feat_len).value, _i32(lens_out).value
    return d, out


def _conv1_ch_desc(feat, w9c, bias, in_ch=1, act=_lib.ACT_RELU, cmvn=None, out=None, feat_len=None, lens_out=None, out_bf16=False):
    """m3_conv1_ch_desc: feat (B, T, idim) read as in_ch blocks of idim / in_ch bins, w9c [in_ch * 9][C]"""
    B, T, idim = feat.shape
    Cc = w9c.shape[1]
    if out is None:
        out = torch.empty(B, (T - 3) // 2 + 1, (idim // max(int(in_ch), 1) - 3) // 2 + 1, Cc,
                          dtype=torch.bfloat16 if out_bf16 else torch.float32, device=feat.device)
    d = _lib.Conv1ChDesc()
    d.feat, d.w9c, d.bias, d.out = _f32(feat).value, _f32(w9c).value, _f32(bias).value, out.data_ptr()
    if cmvn is not None:
        d.cmvn_mean, d.cmvn_istd = _f32(cmvn[0]).value, _f32(cmvn[1]).value
    d.B, d.T, d.idim, d.C, d.act, d.in_ch, d.out_bf16 = B, T, idim, Cc, int(act), int(in_ch), int(out.dtype == torch.bfloat16)
    if feat_len is not None:
        d.feat_len, d.lens_out = _i32(feat_len).value, _i32(lens_out).value
    return d, out


def subsample_conv1_ch(feat, w9c, bias, in_ch, **kw):
    """the first conv with in_ch input channels (m3_subsample_conv1_ch): feat (B, T, idim) -> channel-last (B, T1, F1, C) with
    F1 counted on idim / in_ch; optionally act, cmvn = (mean, istd), out (float32 or bfloat16), out_bf16, feat_len + lens_out"""
    d, out = _conv1_ch_desc(feat, w9c, bias, in_ch, **kw)
    check(_lib.load().m3_subsample_conv1_ch(C.byref(d), _stream()), "m3_subsample_conv1_ch")
    return out


def subsample_conv1_ch_pair(a, b):
    """two such convs on one input shape with one in_ch in one launch (m3_subsample_conv1_ch_pair); a / b: the keyword
    arguments of subsample_conv1_ch (feat_len + lens_out on a only)"""
    (da, oa), (db, ob) = _conv1_ch_desc(**a), _conv1_ch_desc(**b)
    check(_lib.load().m3_subsample_conv1_ch_pair(C.byref(da), C.byref(db), _stream()), "m3_subsample_conv1_ch_pair")
    return oa, ob


def subsample_conv1_pair(a, b):
    """two first convs on inputs of one shape in one launch (m3_subsample_conv1_pair).  Keys of a / b: feat, w9c, bias and
    optionally act, cmvn = (mean, istd), out, feat_len + lens_out (a only)."""
    (da, oa), (db, ob) = _conv1_desc(**a), _conv1_desc(**b)
    check(_lib.load().m3_subsample_conv1_pair(C.byref(da), C.byref(db), _stream()), "m3_subsample_conv1_pair")
    return oa, ob


def subsample_conv1_cmvn(feat, w9c, bias, cmvn, out=None):
    """conv1 + ReLU with global CMVN folded into the read (m3_subsample_conv1_cmvn); cmvn = (mean, istd)"""
    d, out = _conv1_desc(feat, w9c, bias, cmvn=cmvn, out=out)
    check(_lib.load().m3_subsample_conv1_cmvn(d.feat, d.w9c, d.bias, d.cmvn_mean, d.cmvn_istd, d.B, d.T, d.idim, d.C, d.out, _stream()),
          "m3_subsample_conv1_cmvn")
    return out


def layer_norm(x, gamma, beta, eps):
    lib = _lib.load()
    D = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.m3_layer_norm(_f32(x), _f32(gamma), _f32(beta), float(eps), _p(y), x.numel() // D, D, _stream()),
          "m3_layer_norm")
    return y


def relpos_attention(qkv, p, pos_u, pos_v, lens, B, T, H, dk, chunk=0, left_chunks=-1, out=None):
    """chunk > 0: static chunk mask (utils/mask.py:42-75): query i sees keys of its chunk and of `left_chunks` chunks to the
    left (< 0: all) -- besides the padding mask.  qkv (B*T, 3*H*dk), p (T, H*dk) and out (B*T, H*dk) may be row-strided views."""
    lib = _lib.load()
    D = H * dk
    if out is None:
        out = torch.empty(B * T, D, dtype=torch.float32, device=qkv.device)
    assert tuple(qkv.shape) == (B * T, 3 * D) and tuple(p.shape)[1] == D and p.shape[0] >= T and tuple(out.shape) == (B * T, D)
    (qp, ldq), (pp, ldp), (op, ldo) = _rows(qkv), _rows(p), _rows(out)
    if chunk > 0:
        check(lib.m3_relpos_attention_chunk(qp, ldq, pp, ldp, _f32(pos_u), _f32(pos_v), _i32(lens),
                                            B, T, H, dk, 1.0 / math.sqrt(dk), int(chunk), int(left_chunks), op, ldo, _stream()),
              "m3_relpos_attention_chunk")
        return out
    check(lib.m3_relpos_attention(qp, ldq, pp, ldp, _f32(pos_u), _f32(pos_v),
                                  _i32(lens), B, T, H, dk, 1.0 / math.sqrt(dk), op, ldo, _stream()),
          "m3_relpos_attention")
    return out


def relpos_attention_bf16(qkv, p, pos_u, pos_v, lens, B, T, H, dk, chunk=0, left_chunks=-1, out=None):
    """the same on bf16 rows: qkv (B*T, 3*H*dk) bf16 -> ctx (B*T, H*dk) bf16 (T <= 128)"""
    lib = _lib.load()
    D = H * dk
    if out is None:
        out = torch.empty(B * T, D, dtype=torch.bfloat16, device=qkv.device)
    assert tuple(qkv.shape) == (B * T, 3 * D) and tuple(out.shape) == (B * T, D)
    (qp, ldq), (pp, ldp), (op, ldo) = _rows(qkv, torch.bfloat16), _rows(p), _rows(out, torch.bfloat16)
    check(lib.m3_relpos_attention_bf16(qp, ldq, pp, ldp, _f32(pos_u), _f32(pos_v), _i32(lens), B, T, H, dk,
                                       1.0 / math.sqrt(dk), int(chunk), int(left_chunks), op, ldo, _stream()), "m3_relpos_attention_bf16")
    return out


def dwconv_ln_silu(z, w_kc, bias, gamma, beta, eps, B, T, out=None):
    lib = _lib.load()
    K, D = w_kc.shape
    if out is None:
        out = torch.empty_like(z)
    check(lib.m3_dwconv_ln_silu(_f32(z), _f32(w_kc), _f32(bias), _f32(gamma), _f32(beta), float(eps), B, T, D, K,
                                _p(out), _stream()), "m3_dwconv_ln_silu")
    return out


def dwconv_glu_ln_silu(vg, w_kc, bias, gamma, beta, eps, B, T, out=None):
    """Depthwise conv + LayerNorm + SiLU on GLU(vg) formed as the taps are loaded (m3_dwconv_glu_ln_silu): vg (B*T, 2*D) holds
    pointwise_conv1's value | gate columns and may be a row-strided view."""
    lib = _lib.load()
    K, D = w_kc.shape
    assert tuple(vg.shape) == (B * T, 2 * D)
    if out is None:
        out = torch.empty(B * T, D, dtype=torch.float32, device=vg.device)
    vp, ldz = _rows(vg)
    check(lib.m3_dwconv_glu_ln_silu(vp, ldz, _f32(w_kc), _f32(bias), _f32(gamma), _f32(beta), float(eps), B, T, D, K,
                                    _f32(out), _stream()), "m3_dwconv_glu_ln_silu")
    return out


def relpos_attention_stream(qkv, hist, p, pos_u, pos_v, chunk_len, step, B, C, H, dk, left_chunks=-1, slot_max_chunks=-1, out=None):
    """One chunk of the streaming attention (m3_relpos_attention_stream): qkv (B*C, 3*H*dk) and out (B*C, H*dk) may be
    row-strided views, p (p_rows, H*dk) too; hist (B, cap, 2*H*dk) is appended to in place.  step: one int32 on the device
    (lockstep) or int32 [B] with slot_max_chunks >= 0 (slot mode).  The caller advances the counter(s)."""
    lib = _lib.load()
    D = H * dk
    if out is None:
        out = torch.empty(B * C, D, dtype=torch.float32, device=qkv.device)
    assert tuple(qkv.shape) == (B * C, 3 * D) and p.shape[1] == D and tuple(out.shape) == (B * C, D)
    assert hist.dim() == 3 and hist.shape[0] == B and hist.shape[2] == 2 * D
    assert chunk_len.numel() == B and step.numel() == (B if slot_max_chunks >= 0 else 1)
    (qp, ldq), (pp, ldp), (op, ldo) = _rows(qkv), _rows(p), _rows(out)
    check(lib.m3_relpos_attention_stream(qp, ldq, _f32(hist), hist.shape[1], pp, ldp, p.shape[0], _f32(pos_u), _f32(pos_v),
                                         _i32(chunk_len), _i32(step), B, C, H, dk, 1.0 / math.sqrt(dk), int(left_chunks),
                                         int(slot_max_chunks), op, ldo, _stream()), "m3_relpos_attention_stream")
    return out


def dwconv_ln_silu_stream(z, w_kc, bias, gamma, beta, eps, B, T, cache_pair, step, chunk_len, slot_max_chunks=-1, out=None):
    """One chunk of the streaming causal conv + LayerNorm (gamma / beta None: none) + SiLU (m3_dwconv_ln_silu_stream);
    cache_pair (2, B, K-1, D) is the ping-pong state: half (counter & 1) is read, the other half written."""
    lib = _lib.load()
    K, D = w_kc.shape
    assert tuple(cache_pair.shape) == (2, B, K - 1, D) and z.numel() == B * T * D
    assert chunk_len.numel() == B and step.numel() == (B if slot_max_chunks >= 0 else 1)
    if out is None:
        out = torch.empty_like(z)
    check(lib.m3_dwconv_ln_silu_stream(_f32(z), _f32(w_kc), _f32(bias), _f32(gamma), _f32(beta), float(eps), B, T, D, K,
                                       _f32(cache_pair), _i32(step), _i32(chunk_len), int(slot_max_chunks), _f32(out), _stream()),
          "m3_dwconv_ln_silu_stream")
    return out


def dwconv_ln_silu_causal(z, w_kc, bias, gamma, beta, eps, left_fill, B, T, out=None):
    """The causal conv on whole padded utterances (m3_dwconv_ln_silu_causal); left_fill (D,) stands for every frame left of frame 0."""
    lib = _lib.load()
    K, D = w_kc.shape
    assert z.numel() == B * T * D and left_fill.numel() == D
    if out is None:
        out = torch.empty_like(z)
    check(lib.m3_dwconv_ln_silu_causal(_f32(z), _f32(w_kc), _f32(bias), _f32(gamma), _f32(beta), float(eps), _f32(left_fill), B, T, D, K,
                                       _f32(out), _stream()), "m3_dwconv_ln_silu_causal")
    return out


def subsample_conv1(feat, w9c, bias, act=_lib.ACT_RELU, out=None):
    """Conv2d(1, C, 3, stride 2) on (B,T,idim) -> channel-last (B,T1,F1,C); act = ACT_RELU (fused, default) or ACT_NONE."""
    lib = _lib.load()
    B, T, idim = feat.shape
    Cc = w9c.shape[1]
    T1, F1 = (T - 3) // 2 + 1, (idim - 3) // 2 + 1
    if out is None:
        out = torch.empty(B, T1, F1, Cc, dtype=torch.float32, device=feat.device)
    assert tuple(out.shape) == (B, T1, F1, Cc)
    check(lib.m3_conv2d_3x3s2_first(_f32(feat), _f32(w9c), _f32(bias), B, T, idim, Cc, int(act), _p(out), _stream()),
          "m3_conv2d_3x3s2_first")
    return out


def cmvn(x, lens, mean, istd):
    lib = _lib.load()
    B, T, D = x.shape
    y = torch.empty_like(x)
    check(lib.m3_cmvn(_f32(x), _i32(lens), _f32(mean), _f32(istd), B, T, D, _p(y), _stream()), "m3_cmvn")
    return y


def log_softmax_bias(x, bias=None):
    lib = _lib.load()
    n = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.m3_log_softmax_bias(_f32(x), _f32(bias), _p(y), x.numel() // n, n, _stream()), "m3_log_softmax_bias")
    return y


# ---------------------------------------------------------------------------------------- CTC search on the logits
def ctc_greedy(logits, lens=None, blank=0):
    """encoder.py:156-180 on the device: (frame_ids (B,T), tokens (B,T) padded with -1, n_tokens (B,)) int32."""
    lib = _lib.load()
    B, T, V = logits.shape
    dev = logits.device
    ids = torch.empty(B, T, dtype=torch.int32, device=dev)
    tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
    n_tokens = torch.empty(B, dtype=torch.int32, device=dev)
    ln = None if lens is None else lens.reshape(-1).contiguous()
    assert ln is None or ln.numel() == B
    check(lib.m3_ctc_greedy(_f32(logits), _i32(ln), B, T, V, int(blank), _p(ids), _p(tokens), _p(n_tokens), _stream()),
          "m3_ctc_greedy")
    return ids, tokens, n_tokens


def ctc_topk(logits, k):
    """per row log_softmax + k best (value desc, index asc): (top_logp (...,k) f32, top_idx (...,k) i32)."""
    lib = _lib.load()
    V = logits.shape[-1]
    rows = logits.numel() // V
    top_logp = torch.empty(*logits.shape[:-1], k, dtype=torch.float32, device=logits.device)
    top_idx = torch.empty(*logits.shape[:-1], k, dtype=torch.int32, device=logits.device)
    check(lib.m3_ctc_topk(_f32(logits), rows, V, int(k), _p(top_logp), _p(top_idx), _stream()), "m3_ctc_topk")
    return top_logp, top_idx


def ctc_prefix_beam_search_host(top_logp, top_idx, beam, blank=0):
    """encoder.py:232-275 over HOST (T,k) arrays of ctc_topk: [(prefix tuple, score)], best first (native host routine)."""
    import numpy as np
    lib = _lib.load()
    lp = np.ascontiguousarray(top_logp, dtype=np.float32)
    ix = np.ascontiguousarray(top_idx, dtype=np.int32)
    T, k = lp.shape
    assert ix.shape == (T, k)
    toks = np.empty((beam, max(T, 1)), dtype=np.int32)
    hlen = np.empty(beam, dtype=np.int32)
    score = np.empty(beam, dtype=np.float32)
    n = C.c_int32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if T == 0:
        return [(tuple(), 0.0)]
    check(lib.m3_ctc_prefix_beam_search(vp(lp), vp(ix), T, k, int(beam), int(blank), vp(toks), vp(hlen), vp(score),
                                        C.cast(C.byref(n), C.c_void_p)), "m3_ctc_prefix_beam_search")
    return [(tuple(int(v) for v in toks[i, :hlen[i]]), float(score[i])) for i in range(n.value)]


def ctc_beam_desc(B, beam, max_frames, blank=0, k=None):
    """m3_ctc_beam_desc for B utterances (k = beam unless given); raises M3Error on sizes the device search rejects."""
    d = _lib.CtcBeamDesc(int(B), int(beam), int(beam if k is None else k), int(max_frames), int(blank))
    one = _lib.CtcBeamDesc(1, d.beam, d.k, d.max_frames, d.blank)      # B = 0 is a valid (empty) size
    if _lib.load().m3_ctc_beam_state_size(C.byref(one)) == 0:
        raise _lib.M3Error("m3_ctc_beam_state_size failed: " + _lib.last_error())
    return d


# The device search has three forms, each a family of exports: m3_ctc_beam_* (plain), m3_ctc_beam_ctx_* (context biasing, m3asr.context
# builds the images) and m3_ctc_beam_lm_* (biasing + n-gram LM shallow fusion, m3asr.lm builds the images).
def _beam_state_size(name, desc):
    n = getattr(_lib.load(), name)(C.byref(desc))
    if n == 0 and desc.B > 0:
        raise _lib.M3Error(name + " failed: " + _lib.last_error())
    return n


def _beam_reset(family, desc, state, slots):
    """slots: None = every utterance; else an int32 device tensor listing the utterances to restart."""
    name, tail = (family + "_reset", ()) if slots is None else (family + "_reset_slots", (_i32(slots), slots.numel()))
    check(getattr(_lib.load(), name)(C.byref(desc), _p(state), _nbytes(state), *tail, _stream()), name)


def _beam_frames(desc, top_logp, top_idx, n_frames, *per_utterance):
    """the marshalled tail of an advance (top_logp, top_idx, T_chunk, n_frames), behind its shape checks"""
    B, Tc, k = top_logp.shape
    assert B == desc.B and k == desc.k and tuple(top_idx.shape) == (B, Tc, k)
    assert all(t.numel() == B for t in (n_frames,) + per_utterance)
    return _f32(top_logp), _i32(top_idx), Tc, _i32(n_frames)


def _beam_hyps(desc, dev, bonus=False, lm=False):
    """the n-best outputs, in the exports' order: [hyp_tokens, hyp_len, hyp_score, hyp_bonus if bonus, hyp_lm if lm, n_hyps]"""
    B, beam = desc.B, desc.beam
    return ([torch.empty(B, beam, desc.max_frames, dtype=torch.int32, device=dev), torch.empty(B, beam, dtype=torch.int32, device=dev)]
            + [torch.empty(B, beam, dtype=torch.float32, device=dev) for _ in range(1 + bool(bonus) + bool(lm))]
            + [torch.empty(B, dtype=torch.int32, device=dev)])


def _image(image):
    """(pointer, bytes) of a device context image (int32 words; None = no graphs)"""
    return (None, 0) if image is None else (_i32(image), image.numel() * 4)


def ctc_beam_state_size(desc):
    """bytes of device state for desc (host-only call); M3Error on a bad descriptor."""
    return _beam_state_size("m3_ctc_beam_state_size", desc)


def ctc_beam_ctx_state_size(desc):
    """bytes of device state of the biased search: the unbiased layout, then every node's context state and bonus."""
    return _beam_state_size("m3_ctc_beam_ctx_state_size", desc)


def ctc_beam_lm_state_size(desc):
    """bytes of device state of the fused search: the biased layout, then every node's LM state and LM sum."""
    return _beam_state_size("m3_ctc_beam_lm_state_size", desc)


def ctc_beam_reset(desc, state, slots=None):
    """slots: None = every utterance; else an int32 device tensor listing the utterances to restart."""
    _beam_reset("m3_ctc_beam", desc, state, slots)


def ctc_beam_ctx_reset(desc, state, slots=None):
    _beam_reset("m3_ctc_beam_ctx", desc, state, slots)


def ctc_beam_lm_reset(desc, state, slots=None):
    _beam_reset("m3_ctc_beam_lm", desc, state, slots)


def ctc_beam_advance(desc, state, top_logp, top_idx, n_frames):
    """top_logp / top_idx (B, T_chunk, k) from ctc_topk, n_frames (B,) int32 on the device: enqueue, no host sync."""
    frames = _beam_frames(desc, top_logp, top_idx, n_frames)
    check(_lib.load().m3_ctc_beam_advance(C.byref(desc), _p(state), _nbytes(state), *frames, _stream()), "m3_ctc_beam_advance")


def ctc_beam_ctx_advance(desc, state, image, graph_of, top_logp, top_idx, n_frames):
    """ctc_beam_advance with the device image (int32 words, or None) and graph_of (B,) int32 on the device (-1 = unbiased)."""
    frames = _beam_frames(desc, top_logp, top_idx, n_frames, graph_of)
    check(_lib.load().m3_ctc_beam_ctx_advance(C.byref(desc), _p(state), _nbytes(state), *_image(image), _i32(graph_of), *frames,
                                              _stream()), "m3_ctc_beam_ctx_advance")


def ctc_beam_lm_advance(desc, state, image, graph_of, lm_image, lm_on, alpha, beta, top_logp, top_idx, n_frames):
    """ctc_beam_ctx_advance with the device LM image (int32 words, or None), lm_on (B,) int32 on the device (0 = this
    utterance runs without the LM) and the run-time weights alpha (LM) and beta (per token)."""
    frames = _beam_frames(desc, top_logp, top_idx, n_frames, graph_of, lm_on)
    check(_lib.load().m3_ctc_beam_lm_advance(C.byref(desc), _p(state), _nbytes(state), *_image(image), _i32(graph_of),
                                             *_image(lm_image), _i32(lm_on), float(alpha), float(beta), *frames, _stream()),
          "m3_ctc_beam_lm_advance")


def ctc_beam_nbest(desc, state):
    """-> (hyp_tokens (B,beam,max_frames) -1 padded, hyp_len (B,beam), hyp_score (B,beam), n_hyps (B,) -1 = failed), device."""
    out = _beam_hyps(desc, state.device)
    check(_lib.load().m3_ctc_beam_nbest(C.byref(desc), _p(state), _nbytes(state), *map(_p, out), _stream()), "m3_ctc_beam_nbest")
    return tuple(out)


def ctc_beam_ctx_nbest(desc, state, image, graph_of):
    """-> (hyp_tokens, hyp_len, hyp_score (the CTC score), hyp_bonus (B,beam), n_hyps), ordered by CTC score + bonus; device."""
    assert graph_of.numel() == desc.B
    out = _beam_hyps(desc, state.device, bonus=True)
    check(_lib.load().m3_ctc_beam_ctx_nbest(C.byref(desc), _p(state), _nbytes(state), *_image(image), _i32(graph_of), *map(_p, out),
                                            _stream()), "m3_ctc_beam_ctx_nbest")
    return tuple(out)


def ctc_beam_lm_nbest(desc, state, image, graph_of, lm_image, lm_on, alpha, beta, use_eos=True):
    """-> (hyp_tokens, hyp_len, hyp_score (the CTC score), hyp_bonus, hyp_lm (B,beam), n_hyps), ordered by the fused key."""
    assert graph_of.numel() == desc.B and lm_on.numel() == desc.B
    out = _beam_hyps(desc, state.device, bonus=True, lm=True)
    check(_lib.load().m3_ctc_beam_lm_nbest(C.byref(desc), _p(state), _nbytes(state), *_image(image), _i32(graph_of), *_image(lm_image),
                                           _i32(lm_on), float(alpha), float(beta), int(bool(use_eos)), *map(_p, out), _stream()),
          "m3_ctc_beam_lm_nbest")
    return tuple(out)


# ---- context biasing (m3asr.context builds the images)
def ctc_context_validate(image, V):
    """m3_ctc_context_validate on a HOST image (numpy int32 words); raises M3Error naming the first offence."""
    import numpy as np
    img = np.ascontiguousarray(image)
    check(_lib.load().m3_ctc_context_validate(img.ctypes.data_as(C.c_void_p), img.nbytes, int(V)), "m3_ctc_context_validate")


def ctc_prefix_beam_search_ctx_host(top_logp, top_idx, beam, blank=0, image=None, graph=0):
    """ctc_prefix_beam_search_host with the biased ranking of graph `graph` of a HOST image (numpy int32 words; None =
    unbiased): [(prefix tuple, ctc score, bonus = final, context state)], ordered by ctc score + bonus."""
    import numpy as np
    lib = _lib.load()
    lp = np.ascontiguousarray(top_logp, dtype=np.float32)
    ix = np.ascontiguousarray(top_idx, dtype=np.int32)
    T, k = lp.shape
    assert ix.shape == (T, k)
    if T == 0:
        return [(tuple(), 0.0, 0.0, 0)]
    img = None if image is None else np.ascontiguousarray(image)
    toks = np.empty((beam, T), dtype=np.int32)
    hlen = np.empty(beam, dtype=np.int32)
    score = np.empty(beam, dtype=np.float32)
    bonus = np.empty(beam, dtype=np.float32)
    state = np.empty(beam, dtype=np.int32)
    n = C.c_int32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib.m3_ctc_prefix_beam_search_ctx(vp(lp), vp(ix), T, k, int(beam), int(blank), None if img is None else vp(img),
                                            0 if img is None else img.nbytes, int(graph), vp(toks), vp(hlen), vp(score),
                                            vp(bonus), vp(state), C.cast(C.byref(n), C.c_void_p)),
          "m3_ctc_prefix_beam_search_ctx")
    return [(tuple(int(v) for v in toks[i, :hlen[i]]), float(score[i]), float(bonus[i]), int(state[i])) for i in range(n.value)]


# ---- n-gram LM shallow fusion (m3asr.lm builds the images)
def ctc_lm_validate(image, V):
    """m3_ctc_lm_validate on a HOST image (numpy int32 words); raises M3Error naming the first offence."""
    import numpy as np
    img = np.ascontiguousarray(image)
    check(_lib.load().m3_ctc_lm_validate(img.ctypes.data_as(C.c_void_p), img.nbytes, int(V)), "m3_ctc_lm_validate")


def ctc_lm_set_member(image, j):
    """m3_ctc_ngram_set_member on a HOST set (numpy int32 words): (member j's image, a view into `image`; its scale)."""
    import numpy as np
    img = np.ascontiguousarray(image)
    member, nbytes, scale = C.c_void_p(), C.c_size_t(0), C.c_float(0.0)
    check(_lib.load().m3_ctc_ngram_set_member(img.ctypes.data_as(C.c_void_p), img.nbytes, int(j), C.byref(member), C.byref(nbytes),
                                           C.byref(scale)), "m3_ctc_ngram_set_member")
    off = (member.value - img.ctypes.data) // 4
    return img[off:off + nbytes.value // 4], float(scale.value)


def ctc_prefix_beam_search_lm_host(top_logp, top_idx, beam, blank=0, image=None, graph=0, lm_image=None, alpha=0.5, beta=0.0,
                                   use_eos=True):
    """ctc_prefix_beam_search_ctx_host with the fused ranking of a HOST LM image (numpy int32 words; None = no LM):
    [(prefix tuple, ctc score, bonus = context final, lm = log P_LM (+ final with use_eos), context state)], ordered by
    (ctc + bonus) + (alpha lm + beta len)."""
    import numpy as np
    lib = _lib.load()
    lp = np.ascontiguousarray(top_logp, dtype=np.float32)
    ix = np.ascontiguousarray(top_idx, dtype=np.int32)
    T, k = lp.shape
    assert ix.shape == (T, k)
    if T == 0:
        return [(tuple(), 0.0, 0.0, 0.0, 0)]
    img = None if image is None else np.ascontiguousarray(image)
    lmi = None if lm_image is None else np.ascontiguousarray(lm_image)
    toks = np.empty((beam, T), dtype=np.int32)
    hlen = np.empty(beam, dtype=np.int32)
    score = np.empty(beam, dtype=np.float32)
    bonus = np.empty(beam, dtype=np.float32)
    lm = np.zeros(beam, dtype=np.float32)
    state = np.empty(beam, dtype=np.int32)
    n = C.c_int32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib.m3_ctc_prefix_beam_search_lm(vp(lp), vp(ix), T, k, int(beam), int(blank), None if img is None else vp(img),
                                           0 if img is None else img.nbytes, int(graph), None if lmi is None else vp(lmi),
                                           0 if lmi is None else lmi.nbytes, float(alpha), float(beta), int(bool(use_eos)),
                                           vp(toks), vp(hlen), vp(score), vp(bonus), vp(state), vp(lm),
                                           C.cast(C.byref(n), C.c_void_p)), "m3_ctc_prefix_beam_search_lm")
    return [(tuple(int(v) for v in toks[i, :hlen[i]]), float(score[i]), float(bonus[i]), float(lm[i]), int(state[i]))
            for i in range(n.value)]


# ---- WFST decoding (m3asr.wfst builds the graph images)
def wfst_validate(image, V):
    """m3_wfst_validate on a HOST image (numpy int32 words); raises M3Error naming the first offence."""
    import numpy as np
    img = np.ascontiguousarray(image)
    check(_lib.load().m3_wfst_validate(img.ctypes.data_as(C.c_void_p), img.nbytes, int(V)), "m3_wfst_validate")


def wfst_search_state_size(desc):
    """bytes of device state for desc (host-only call); M3Error on a bad descriptor."""
    n = _lib.load().m3_wfst_search_state_size(C.byref(desc))
    if n == 0 and desc.B > 0:
        raise _lib.M3Error("m3_wfst_search_state_size failed: " + _lib.last_error())
    return n


def wfst_search_reset(desc, state, graph, slots=None):
    """graph: the device image (int32 words); slots: None = every utterance, else an int32 device tensor."""
    check(_lib.load().m3_wfst_search_reset(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(graph),
                                           graph.numel() * 4, _i32(slots), 0 if slots is None else slots.numel(), _stream()),
          "m3_wfst_search_reset")


def wfst_search_advance(desc, state, graph, logp, n_frames):
    """logp (B, T_chunk, V) float32 log-probabilities with unit column stride and dense frames, n_frames (B,) int32, device."""
    B, Tc, V = logp.shape
    assert B == desc.B and V == desc.V and n_frames.numel() == B and logp.is_cuda and logp.dtype == torch.float32
    assert logp.stride(2) == 1 and logp.stride(0) == Tc * logp.stride(1), "logp: (B, T, V) rows with one leading dimension"
    check(_lib.load().m3_wfst_search_advance(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(graph),
                                             graph.numel() * 4, C.c_void_p(logp.data_ptr()), logp.stride(1), Tc, _i32(n_frames),
                                             _stream()), "m3_wfst_search_advance")


def wfst_search_result(desc, state, graph, final=True, max_words=1, out=None):
    """-> (words (B, max_words) -1 padded, frames (B, max_words), n_words (B,), cost (B,) f32, reached_final (B,), status (B,)),
    device.  out: the six tensors to write into (the tests pass guarded ones)."""
    dev, B = state.device, desc.B
    if out is None:
        out = (torch.empty(B, max_words, dtype=torch.int32, device=dev), torch.empty(B, max_words, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    words, frames, n_words, cost, flags, status = out
    check(_lib.load().m3_wfst_search_result(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(graph),
                                            graph.numel() * 4, int(bool(final)), int(max_words), _i32(words), _i32(frames),
                                            _i32(n_words), _f32(cost), _i32(flags), _i32(status), _stream()), "m3_wfst_search_result")
    return out


# ---- CTC blank-frame skipping in front of the WFST search (m3_wfst_skip_*; m3asr.wfst.CtcWfstSearch(blank_skip=) drives these)
def wfst_skip_desc(B, V, blank, max_frames, log_blank_thresh):
    """m3_wfst_skip_desc.  Raises M3Error on a descriptor the library refuses (host-only call)."""
    d = _lib.WfstSkipDesc(int(B), int(V), int(blank), int(max_frames), float(log_blank_thresh))
    one = _lib.WfstSkipDesc.from_buffer_copy(d)                        # B = 0 is a valid (empty) size
    one.B = 1
    if d.B < 0 or _lib.load().m3_wfst_skip_state_size(C.byref(one)) == 0:
        raise _lib.M3Error("m3_wfst_skip_state_size failed: " + (_lib.last_error() if d.B >= 0 else "B = %d" % d.B))
    return d


def wfst_skip_state_size(desc):
    """bytes of device state for desc (host-only call); M3Error on a bad descriptor."""
    n = _lib.load().m3_wfst_skip_state_size(C.byref(desc))
    if n == 0 and desc.B > 0:
        raise _lib.M3Error("m3_wfst_skip_state_size failed: " + _lib.last_error())
    return n


def wfst_skip_reset(desc, state, slots=None):
    """slots: None = every utterance, else an int32 device tensor."""
    check(_lib.load().m3_wfst_skip_reset(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(slots),
                                         0 if slots is None else slots.numel(), _stream()), "m3_wfst_skip_reset")


def wfst_skip_select(desc, state, logp, n_frames, out, n_kept):
    """logp (B, T_chunk, >= V) and out (B, T_chunk + 1, >= V) float32 device views with unit column stride and dense frames (the
    row stride is passed as ld / ld_out), n_frames / n_kept (B,) int32 on the device.  Enqueues, no host sync."""
    B, Tc = logp.shape[0], logp.shape[1]
    assert B == desc.B and n_frames.numel() == B and n_kept.numel() == B and logp.is_cuda and out.is_cuda
    assert logp.dtype == torch.float32 and out.dtype == torch.float32 and out.shape[0] == B and out.shape[1] == Tc + 1
    for t, rows in ((logp, Tc), (out, Tc + 1)):
        assert t.stride(2) == 1 and (B <= 1 or t.stride(0) == rows * t.stride(1)), "(B, T, V) rows with one leading dimension"
    check(_lib.load().m3_wfst_skip_select(C.byref(desc), _p(state), state.numel() * state.element_size(),
                                          C.c_void_p(logp.data_ptr()), logp.stride(1), Tc, _i32(n_frames),
                                          C.c_void_p(out.data_ptr()), out.stride(1), _i32(n_kept), _stream()), "m3_wfst_skip_select")


def wfst_skip_map_frames(desc, state, frames, n_words):
    """frames (B, ld_frames) int32 in place, n_words (B,) int32, device: decoded frame numbers -> real ones."""
    assert frames.dim() == 2 and frames.shape[0] == desc.B and n_words.numel() == desc.B
    check(_lib.load().m3_wfst_skip_map_frames(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(frames),
                                              frames.shape[1], _i32(n_words), _stream()), "m3_wfst_skip_map_frames")
    return frames


def wfst_skip_counts(desc, state, out=None):
    """-> (seen (B,), kept (B,)) int32 on the device: frames seen / emitted since each utterance's reset."""
    if out is None:
        out = (torch.empty(desc.B, dtype=torch.int32, device=state.device), torch.empty(desc.B, dtype=torch.int32, device=state.device))
    check(_lib.load().m3_wfst_skip_counts(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(out[0]), _i32(out[1]),
                                          _stream()), "m3_wfst_skip_counts")
    return out


def ctc_greedy_stream_desc(B, max_frames, blank=0):
    d = _lib.CtcGreedyDesc(int(B), int(max_frames), int(blank))
    if _lib.load().m3_ctc_greedy_stream_state_size(C.byref(_lib.CtcGreedyDesc(1, d.max_frames, d.blank))) == 0:
        raise _lib.M3Error("m3_ctc_greedy_stream_state_size failed: " + _lib.last_error())
    return d


def ctc_greedy_stream_state_size(desc):
    return _lib.load().m3_ctc_greedy_stream_state_size(C.byref(desc))


def ctc_greedy_stream_reset(desc, state, slots=None):
    if slots is not None:
        check(_lib.load().m3_ctc_greedy_stream_reset_slots(C.byref(desc), _p(state), state.numel() * state.element_size(),
                                                           _i32(slots), slots.numel(), _stream()), "m3_ctc_greedy_stream_reset_slots")
        return
    check(_lib.load().m3_ctc_greedy_stream_reset(C.byref(desc), _p(state), state.numel() * state.element_size(), _stream()),
          "m3_ctc_greedy_stream_reset")


def ctc_greedy_stream_advance(desc, state, logits, n_frames, frame_ids=None):
    """logits (B, T_chunk, V) f32, n_frames (B,) int32 on the device; frame_ids: optional (B, T_chunk) int32 scratch."""
    B, Tc, V = logits.shape
    assert B == desc.B and n_frames.numel() == B
    if frame_ids is None:
        frame_ids = torch.empty(B, Tc, dtype=torch.int32, device=logits.device)
    check(_lib.load().m3_ctc_greedy_stream_advance(C.byref(desc), _p(state), state.numel() * state.element_size(), _f32(logits),
                                                   Tc, V, _i32(n_frames), _i32(frame_ids), _stream()),
          "m3_ctc_greedy_stream_advance")
    return frame_ids


def ctc_greedy_stream_tokens(desc, state):
    """-> (tokens (B, max_frames) -1 padded, n_tokens (B,) -1 = failed), device int32."""
    tokens = torch.empty(desc.B, desc.max_frames, dtype=torch.int32, device=state.device)
    n = torch.empty(desc.B, dtype=torch.int32, device=state.device)
    check(_lib.load().m3_ctc_greedy_stream_tokens(C.byref(desc), _p(state), state.numel() * state.element_size(), _p(tokens),
                                                  _p(n), _stream()), "m3_ctc_greedy_stream_tokens")
    return tokens, n


# ---- endpoint detection (m3asr.decode.EndpointConfig builds the descriptor)
def ctc_endpoint_desc(B, blank, log_blank_threshold, rules):
    """m3_ctc_endpoint_desc for B streams; rules: up to four (must_decoded, min_trailing frames, min_length frames);
    log_blank_threshold: a float32 in [log 0.5, 0).  Raises M3Error on a descriptor the library rejects."""
    if len(rules) > 4:
        raise _lib.M3Error("ctc_endpoint_desc: %d rules, at most 4" % len(rules))
    d = _lib.CtcEndpointDesc()
    d.B, d.blank, d.n_rules, d.log_blank_threshold = int(B), int(blank), len(rules), float(log_blank_threshold)
    for r, (must, trail, length) in enumerate(rules):
        d.rule[r].must_decoded, d.rule[r].min_trailing, d.rule[r].min_length = int(bool(must)), int(trail), int(length)
    one = _lib.CtcEndpointDesc.from_buffer_copy(d)                     # B = 0 is a valid (empty) size
    one.B = 1
    if _lib.load().m3_ctc_endpoint_state_size(C.byref(one)) == 0:
        raise _lib.M3Error("m3_ctc_endpoint_state_size failed: " + _lib.last_error())
    return d


def ctc_endpoint_state_size(desc):
    n = _lib.load().m3_ctc_endpoint_state_size(C.byref(desc))
    if n == 0 and desc.B > 0:
        raise _lib.M3Error("m3_ctc_endpoint_state_size failed: " + _lib.last_error())
    return n


def ctc_endpoint_reset(desc, state, slots=None):
    """slots: None = every stream; else an int32 device tensor listing the streams to restart."""
    if slots is not None:
        check(_lib.load().m3_ctc_endpoint_reset_slots(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(slots),
                                                      slots.numel(), _stream()), "m3_ctc_endpoint_reset_slots")
        return
    check(_lib.load().m3_ctc_endpoint_reset(C.byref(desc), _p(state), state.numel() * state.element_size(), _stream()),
          "m3_ctc_endpoint_reset")


def ctc_endpoint_advance(desc, state, top_logp, top_idx, n_frames):
    """top_logp / top_idx (B, T_chunk, k) from ctc_topk (any k >= 1), n_frames (B,) int32 on the device: enqueue, no host sync."""
    B, Tc, k = top_logp.shape
    assert B == desc.B and tuple(top_idx.shape) == (B, Tc, k) and n_frames.numel() == B
    check(_lib.load().m3_ctc_endpoint_advance(C.byref(desc), _p(state), state.numel() * state.element_size(), _f32(top_logp),
                                              _i32(top_idx), Tc, k, _i32(n_frames), _stream()), "m3_ctc_endpoint_advance")


def ctc_endpoint_read(desc, state, info=None):
    """-> info (B, 8) int32 on the device: frames, trailing_blank, decoded, first_speech, last_speech, fired_rule, fired_frame, 0."""
    if info is None:
        info = torch.empty(desc.B, 8, dtype=torch.int32, device=state.device)
    assert tuple(info.shape) == (desc.B, 8)
    check(_lib.load().m3_ctc_endpoint_read(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(info), _stream()),
          "m3_ctc_endpoint_read")
    return info


# ---- attention rescoring (m3asr.rescore drives these around the decoder's GEMMs)
def aed_embed(hyp_tokens, hyp_len, n_hyps, hyp_row0, emb, pe, rows, reverse=False):
    """Decoder input rows of the device n-best (m3_aed_embed): hyp_tokens (B,beam,max_frames), hyp_len (B,beam), n_hyps (B,),
    hyp_row0 (B*beam+1,) int32; emb (V,D), pe (pe_rows,D) -> (x (rows,D) f32, target (rows,) int32)."""
    B, beam, F = hyp_tokens.shape
    V, D = emb.shape
    assert hyp_row0.numel() == B * beam + 1 and hyp_len.numel() == B * beam and n_hyps.numel() == B and pe.shape[1] == D
    x = torch.empty(rows, D, dtype=torch.float32, device=emb.device)
    target = torch.empty(rows, dtype=torch.int32, device=emb.device)
    check(_lib.load().m3_aed_embed(_i32(hyp_tokens), _i32(hyp_len), _i32(n_hyps), _i32(hyp_row0), B, beam, F, _f32(emb), _f32(pe),
                                   pe.shape[0], V, D, int(bool(reverse)), int(rows), _p(x), D, _p(target), _stream()), "m3_aed_embed")
    return x, target


def aed_attention(q, k, v, desc, max_q, H, out=None):
    """Multi-head attention core on packed query rows (m3_aed_attention): q (q_rows, H*dk), k / v (kv_rows, H*dk) row-strided
    views, desc (n_slots, 5) int32 = (q_row0, n_q, kv_row0, kv_len, causal) per hypothesis slot -> ctx (q_rows, H*dk)."""
    D = q.shape[1]
    dk = D // H
    assert D == H * dk and k.shape[1] == D and v.shape[1] == D and k.shape[0] == v.shape[0]
    assert desc.dim() == 2 and desc.shape[1] == 5
    if out is None:
        out = torch.empty(q.shape[0], D, dtype=torch.float32, device=q.device)
    (qp, ldq), (kp, ldk), (vp, ldv), (op, ldo) = _rows(q), _rows(k), _rows(v), _rows(out)
    check(_lib.load().m3_aed_attention(qp, ldq, kp, ldk, vp, ldv, _i32(desc), desc.shape[0], int(max_q), q.shape[0], k.shape[0],
                                       H, dk, 1.0 / math.sqrt(dk), op, ldo, _stream()), "m3_aed_attention")
    return out


def aed_score(logits, target, hyp_row0, n_hyps, B, beam, prior=None, ctc_weight=0.0, r_logits=None, r_target=None,
              reverse_weight=0.0):
    """Scores and choice (m3_aed_score): logits (rows, V) [+ r_logits of the right-to-left decoder] ->
    (att, r_att, final (B,beam) f32, best (B,) int32); dead slots hold -inf, best = -1 without hypotheses."""
    rows, V = logits.shape
    dev = logits.device
    att = torch.empty(B, beam, dtype=torch.float32, device=dev)
    r_att, final = torch.empty_like(att), torch.empty_like(att)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(2 * rows, 1), dtype=torch.float32, device=dev)
    (lp, ldl) = _rows(logits) if rows else (None, V)
    (rp, ldrl) = _rows(r_logits) if (r_logits is not None and rows) else (None, V)
    assert r_logits is None or tuple(r_logits.shape) == (rows, V)
    check(_lib.load().m3_aed_score(lp, ldl, rp, ldrl, _i32(target) if rows else None,
                                   _i32(r_target) if (r_logits is not None and rows) else None, _i32(hyp_row0), _i32(n_hyps),
                                   _f32(prior), B, beam, rows, V, float(ctc_weight), float(reverse_weight), _p(scratch), _p(att),
                                   _p(r_att), _p(final), _p(best), _stream()), "m3_aed_score")
    return att, r_att, final, best


# ---- per-slot encoder memory of streaming two-pass decoding (m3_aed_memory_*; StreamingCtcDecoder(rescorer=) drives these)
def aed_memory_desc(B, max_frames, D):
    """m3_aed_memory_desc for B streams of at most max_frames rows of D floats.  Raises M3Error on a descriptor the library
    rejects (D no multiple of 4, a negative size)."""
    d = _lib.AedMemoryDesc(int(B), int(max_frames), int(D))
    if _lib.load().m3_aed_memory_state_size(C.byref(_lib.AedMemoryDesc(1, d.max_frames, d.D))) == 0 or d.B < 0:
        raise _lib.M3Error("m3_aed_memory_state_size failed: " + (_lib.last_error() if d.B >= 0 else "B = %d" % d.B))
    return d


def aed_memory_state_size(desc):
    return _lib.load().m3_aed_memory_state_size(C.byref(desc))


def aed_memory_reset(desc, state, slots=None):
    """slots: None = every stream; else an int32 device tensor listing the streams to restart."""
    if slots is not None:
        check(_lib.load().m3_aed_memory_reset_slots(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(slots),
                                                    slots.numel(), _stream()), "m3_aed_memory_reset_slots")
        return
    check(_lib.load().m3_aed_memory_reset(C.byref(desc), _p(state), state.numel() * state.element_size(), _stream()),
          "m3_aed_memory_reset")


def aed_memory_append(desc, state, x, n_frames):
    """x (B * T_chunk, D) f32 rows of the chunk (a row-strided view is fine), n_frames (B,) int32 on the device: enqueue, no
    host sync."""
    xp, ldx = _rows(x)
    assert x.shape[1] == desc.D and x.shape[0] % max(desc.B, 1) == 0 and n_frames.numel() == desc.B
    check(_lib.load().m3_aed_memory_append(C.byref(desc), _p(state), state.numel() * state.element_size(), xp, ldx,
                                           x.shape[0] // max(desc.B, 1), _i32(n_frames), _stream()), "m3_aed_memory_append")


def aed_memory_lengths(desc, state):
    """-> (B,) int32 on the device: rows every stream holds, -1 for a stream that ran past max_frames."""
    n = torch.empty(desc.B, dtype=torch.int32, device=state.device)
    check(_lib.load().m3_aed_memory_lengths(C.byref(desc), _p(state), state.numel() * state.element_size(), _p(n), _stream()),
          "m3_aed_memory_lengths")
    return n


def aed_memory_gather(desc, state, slots, out=None):
    """The listed streams' rows packed in list order: slots (n,) int32 on the device -> (out (rows, D), row0 (n + 1,) int32 on
    the device); the first row0[n] rows of `out` are written.  out: a row-strided (rows, D) view to fill (default: a fresh
    (n * max_frames, D) buffer, which holds whatever the streams have)."""
    n = slots.numel()
    if out is None:
        out = torch.empty(n * desc.max_frames, desc.D, dtype=torch.float32, device=state.device)
    assert out.dim() == 2 and out.shape[1] == desc.D
    row0 = torch.empty(n + 1, dtype=torch.int32, device=state.device)
    (op, ldo) = _rows(out) if out.shape[0] else (None, desc.D)
    check(_lib.load().m3_aed_memory_gather(C.byref(desc), _p(state), state.numel() * state.element_size(), _i32(slots), n, op, ldo,
                                           out.shape[0], _p(row0), _stream()), "m3_aed_memory_gather")
    return out, row0


# ---- CTC forced alignment (m3_ctc_align_*; m3asr.align.CtcAligner drives these)
def ctc_align_desc(n, V, blank, max_frames, max_tokens):
    """m3_ctc_align_desc for n packed utterances of at most max_frames frames and max_tokens tokens.  Raises M3Error on a
    descriptor the library refuses (blank outside [0, V), more than 4000 tokens, sizes that overflow the int32 arithmetic)."""
    d = _lib.CtcAlignDesc(int(n), int(V), int(blank), int(max_frames), int(max_tokens))
    if _lib.load().m3_ctc_align_workspace_size(C.byref(d)) == 0:
        raise _lib.M3Error("m3_ctc_align_workspace_size failed: " + _lib.last_error())
    return d


def ctc_align_workspace_size(desc):
    """bytes of the move table for desc (host-only call); 0 for a descriptor the library refuses."""
    return _lib.load().m3_ctc_align_workspace_size(C.byref(desc))


def ctc_align_emit(desc, rows, row0, n_frames, tokens, tok0, emit=None):
    """rows (R, V) f32 logits (a row-strided view is fine), row0 / n_frames (n,), tokens (sum L,), tok0 (n + 1,) int32 on the
    device -> emit (n, max_frames, max_tokens + 1) f32: the log-probabilities of the blank and of each utterance's tokens
    (rows t < n_frames and columns <= L are written)."""
    xp, ldl = _rows(rows)
    assert rows.shape[1] == desc.V and row0.numel() == n_frames.numel() == desc.n and tok0.numel() == desc.n + 1
    if emit is None:
        emit = torch.empty(desc.n, desc.max_frames, desc.max_tokens + 1, dtype=torch.float32, device=rows.device)
    check(_lib.load().m3_ctc_align_emit(C.byref(desc), xp, ldl, _i32(row0), _i32(n_frames), _i32(tokens), _i32(tok0), _f32(emit),
                                        _stream()), "m3_ctc_align_emit")
    return emit


def ctc_align_path(desc, emit, n_frames, tokens, tok0, workspace, out=None):
    """The trellis, the backtrace and the spans on `emit` -> (score (n,) f32, status (n,), state (n, max_frames), tok_start,
    tok_end, tok_peak (sum L,) int32, tok_logp (sum L,) f32) on the device.  out: that tuple, to be filled."""
    dev = emit.device
    if out is None:
        nt = tokens.numel()
        out = (torch.empty(desc.n, dtype=torch.float32, device=dev), torch.empty(desc.n, dtype=torch.int32, device=dev),
               torch.empty(desc.n, desc.max_frames, dtype=torch.int32, device=dev)) + \
            tuple(torch.empty(nt, dtype=torch.int32, device=dev) for _ in range(3)) + (torch.empty(nt, dtype=torch.float32, device=dev),)
    score, status, state, ts, te, tp, tl = out
    check(_lib.load().m3_ctc_align_path(C.byref(desc), _f32(emit), _i32(n_frames), _i32(tokens), _i32(tok0), _p(workspace),
                                        workspace.numel() * workspace.element_size(), _f32(score), _i32(status), _i32(state),
                                        _i32(ts), _i32(te), _i32(tp), _f32(tl), _stream()), "m3_ctc_align_path")
    return out


# ---- attention decoding: the AED decoder's own beam search (m3_aed_search_*; m3asr.aed_search drives these around the GEMMs)
def aed_search_desc(B, beam, max_steps, V, D, H, layers, pe_rows):
    """m3_aed_search_desc.  Raises M3Error on a descriptor the library rejects (beam outside [1, min(64, V)], a head size that
    is no multiple of 16 up to 128, sizes that overflow the int32 row arithmetic of the state or of the K / V cache)."""
    d = _lib.AedSearchDesc(int(B), int(beam), int(max_steps), int(V), int(D), int(H), int(layers), int(pe_rows))
    if d.B < 1:
        raise _lib.M3Error("aed_search_desc: B = %d, need at least one utterance" % d.B)
    if _lib.load().m3_aed_search_state_size(C.byref(d)) == 0:
        raise _lib.M3Error("m3_aed_search_state_size failed: " + _lib.last_error())
    return d


def aed_search_state_size(desc):
    return _lib.load().m3_aed_search_state_size(C.byref(desc))


def aed_search_cache_size(desc):
    """bytes of the self-attention K / V cache: layers * max_steps * B * beam * 2 D fp32"""
    return _lib.load().m3_aed_search_cache_size(C.byref(desc))


def _nbytes(t):
    return t.numel() * t.element_size()


def aed_search_reset(desc, state, mem_row0, mem_len, max_steps=None):
    """mem_row0 / mem_len (B,) int32 on the device: the memory rows of every utterance; max_steps <= desc.max_steps"""
    assert mem_row0.numel() == desc.B and mem_len.numel() == desc.B
    check(_lib.load().m3_aed_search_reset(C.byref(desc), _p(state), _nbytes(state), _i32(mem_row0), _i32(mem_len),
                                          int(desc.max_steps if max_steps is None else max_steps), _stream()), "m3_aed_search_reset")


def aed_search_embed(desc, state, emb, pe, x):
    """x (R, D) <- emb[last token] * sqrt(D) + pe[step], from the state"""
    assert tuple(emb.shape) == (desc.V, desc.D) and tuple(pe.shape) == (desc.pe_rows, desc.D)
    xp, ldx = _rows(x)
    assert tuple(x.shape) == (desc.B * desc.beam, desc.D)
    check(_lib.load().m3_aed_search_embed(C.byref(desc), _p(state), _nbytes(state), _f32(emb), _f32(pe), xp, ldx, _stream()),
          "m3_aed_search_embed")
    return x


def aed_search_attention(desc, state, q, kv, out, layer, cache=None):
    """Single-query attention of the R hypothesis rows (m3_aed_search_attention).  q (R, D) and kv (rows, 2 D) = K | V are
    row-strided views.  cache given: self use, kv = the rows' new K | V (qkv[:, D:]), stored at the step's cache position;
    cache None: source use, kv = the memory's projection for `layer`."""
    R = desc.B * desc.beam
    (qp, ldq), (kp, ldkv), (op, ldo) = _rows(q), _rows(kv), _rows(out)
    assert tuple(q.shape) == (R, desc.D) and tuple(out.shape) == (R, desc.D) and kv.shape[1] == 2 * desc.D
    check(_lib.load().m3_aed_search_attention(C.byref(desc), _p(state), _nbytes(state), qp, ldq, kp, ldkv, kv.shape[0],
                                              _f32(cache), _nbytes(cache) if cache is not None else 0, int(layer), op, ldo,
                                              _stream()), "m3_aed_search_attention")
    return out


def aed_search_prune(desc, state, logits, done=None):
    """One search step's log-softmax, top-k, prune and bookkeeping over logits (R, V); done (B,) int32 receives the flags"""
    lp, ldl = _rows(logits)
    assert tuple(logits.shape) == (desc.B * desc.beam, desc.V) and (done is None or done.numel() == desc.B)
    check(_lib.load().m3_aed_search_prune(C.byref(desc), _p(state), _nbytes(state), lp, ldl, _i32(done), _stream()),
          "m3_aed_search_prune")


def aed_search_result(desc, state):
    """-> dict(hyp_tokens (B,beam,max_steps), hyp_len, score, finished (B,beam), best, steps (B,)) on the device"""
    B, N, dev = desc.B, desc.beam, state.device
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)   # noqa: E731
    out = dict(hyp_tokens=i32(B, N, desc.max_steps), hyp_len=i32(B, N), score=torch.empty(B, N, dtype=torch.float32, device=dev),
               finished=i32(B, N), best=i32(B), steps=i32(B))
    check(_lib.load().m3_aed_search_result(C.byref(desc), _p(state), _nbytes(state), _p(out["hyp_tokens"]), _p(out["hyp_len"]),
                                           _p(out["score"]), _p(out["finished"]), _p(out["best"]), _p(out["steps"]), _stream()),
          "m3_aed_search_result")
    return out


# ---- joint CTC/attention decoding: CTC prefix scores inside that search (m3_aed_joint_*)
def _aed_fused_desc(search_desc, pre_beam, max_frames, size_fn):
    """m3_aed_joint_desc around a search descriptor, validated by the size function of the family that will use it"""
    d = _lib.AedJointDesc(search_desc, int(pre_beam), int(max_frames))
    if getattr(_lib.load(), size_fn)(C.byref(d)) == 0:
        raise _lib.M3Error(size_fn + " failed: " + _lib.last_error())
    return d


def _blobs(*blobs):
    """optional uint8 blobs -> pointer, bytes, pointer, bytes, ...; None: NULL, 0"""
    return [v for t in blobs for v in (_p(t), _nbytes(t) if t is not None else 0)]


def _opt_rows(t):
    """an optional row-strided (rows, n) float input -> pointer, ld, rows; None: NULL, 0, 0"""
    return (None, 0, 0) if t is None else _rows(t) + (t.shape[0],)


def aed_joint_desc(search_desc, pre_beam, max_frames):
    """m3_aed_joint_desc around a search descriptor.  Raises M3Error on what the library rejects (pre_beam outside
    [beam, min(64, V)], max_frames < 1, V < 2, sizes that overflow the int32 offsets of the scorer state or the scratch)."""
    return _aed_fused_desc(search_desc, pre_beam, max_frames, "m3_aed_joint_state_size")


def aed_joint_state_size(desc):
    return _lib.load().m3_aed_joint_state_size(C.byref(desc))


def aed_joint_scratch_size(desc):
    return _lib.load().m3_aed_joint_scratch_size(C.byref(desc))


def aed_joint_reset(desc, state, jstate, ctc):
    """after aed_search_reset: the scorer state of the empty hypothesis from ctc (rows, V) log-probabilities"""
    cp, ldc = _rows(ctc)
    check(_lib.load().m3_aed_joint_reset(C.byref(desc), _p(state), _nbytes(state), _p(jstate), _nbytes(jstate), cp, ldc, ctc.shape[0],
                                         _stream()), "m3_aed_joint_reset")


def aed_joint_score(desc, state, jstate, scratch, logits, ctc, ctc_weight):
    """per row: log-softmax of logits (R, V), the pre_beam picks and every pick's CTC prefix score -> the candidate scratch"""
    (lp, ldl), (cp, ldc) = _rows(logits), _rows(ctc)
    assert tuple(logits.shape) == (desc.search.B * desc.search.beam, desc.search.V) and ctc.shape[1] == desc.search.V
    check(_lib.load().m3_aed_joint_score(C.byref(desc), _p(state), _nbytes(state), _p(jstate), _nbytes(jstate), _p(scratch),
                                         _nbytes(scratch), lp, ldl, cp, ldc, ctc.shape[0], float(ctc_weight), _stream()),
          "m3_aed_joint_score")


def aed_joint_prune(desc, state, jstate, scratch, done=None):
    """the beam best keys of the scratch's candidates; records, paths, parts and scorer states move to the other buffer"""
    assert done is None or done.numel() == desc.search.B
    check(_lib.load().m3_aed_joint_prune(C.byref(desc), _p(state), _nbytes(state), _p(jstate), _nbytes(jstate), _p(scratch),
                                         _nbytes(scratch), _i32(done), _stream()), "m3_aed_joint_prune")


def aed_joint_result(desc, state, jstate):
    """-> dict(att, ctc (B, beam)) on the device: the two parts of the keys aed_search_result returns as scores"""
    B, N = desc.search.B, desc.search.beam
    out = dict(att=torch.empty(B, N, dtype=torch.float32, device=state.device), ctc=torch.empty(B, N, dtype=torch.float32, device=state.device))
    check(_lib.load().m3_aed_joint_result(C.byref(desc), _p(state), _nbytes(state), _p(jstate), _nbytes(jstate), _p(out["att"]),
                                          _p(out["ctc"]), _stream()), "m3_aed_joint_result")
    return out


# ---- n-gram LM fusion and a length bonus in that search (m3_aed_ngram_*)
def aed_lm_desc(search_desc, pre_beam, max_frames=0):
    """The descriptor of the fused search: m3_aed_joint_desc; max_frames = 0 where there is no CTC part (ctc_weight = 0).
    Raises M3Error on what the library rejects."""
    return _aed_fused_desc(search_desc, pre_beam, max_frames, "m3_aed_ngram_state_size")


def aed_lm_state_size(desc):
    return _lib.load().m3_aed_ngram_state_size(C.byref(desc))


def aed_lm_scratch_size(desc):
    return _lib.load().m3_aed_ngram_scratch_size(C.byref(desc))


def aed_lm_reset(desc, lstate, lm_image):
    """after aed_search_reset (and aed_joint_reset): every slot in the image's start state; refuses an image of another V"""
    lmi, lm_bytes = _image(lm_image)
    check(_lib.load().m3_aed_ngram_reset(C.byref(desc), _p(lstate), _nbytes(lstate), lmi, lm_bytes, _stream()), "m3_aed_ngram_reset")


def aed_lm_reset_set(desc, lstate, lm_image, lm_on):
    """m3_aed_ngram_reset_set: aed_lm_reset for an LM set; lm_on (B,) int32 on the device picks each utterance's member, whose
    start state its slots get."""
    assert lm_on.numel() == desc.search.B
    lmi, lm_bytes = _image(lm_image)
    check(_lib.load().m3_aed_ngram_reset_set(C.byref(desc), _p(lstate), _nbytes(lstate), lmi, lm_bytes, _i32(lm_on), _stream()),
          "m3_aed_ngram_reset_set")


def aed_lm_score(desc, state, jstate, scratch, lstate, lscratch, logits, ctc, ctc_weight, lm_image, lm_on, alpha, beta, use_eos=True):
    """aed_joint_score with every candidate's LM step and the fused key; ctc / jstate / scratch None exactly when ctc_weight = 0"""
    assert tuple(logits.shape) == (desc.search.B * desc.search.beam, desc.search.V) and lm_on.numel() == desc.search.B
    check(_lib.load().m3_aed_ngram_score(C.byref(desc), *_blobs(state, jstate, scratch, lstate, lscratch), *_rows(logits), *_opt_rows(ctc),
                                      float(ctc_weight), *_image(lm_image), _i32(lm_on), float(alpha), float(beta), int(bool(use_eos)),
                                      _stream()), "m3_aed_ngram_score")


def aed_lm_prune(desc, state, jstate, scratch, lstate, lscratch, done=None):
    """aed_joint_prune, the survivors' LM state copied from the LM scratch; jstate / scratch None: the search without CTC"""
    assert done is None or done.numel() == desc.search.B
    check(_lib.load().m3_aed_ngram_prune(C.byref(desc), *_blobs(state, jstate, scratch, lstate, lscratch), _i32(done), _stream()),
          "m3_aed_ngram_prune")


def aed_lm_result(desc, state, lstate):
    """-> dict(lm (B, beam) float32, lm_state, lm_n (B, beam) int32, lm_att (B, beam) float32) on the device"""
    B, N, dev = desc.search.B, desc.search.beam, state.device
    out = dict(lm=torch.empty(B, N, dtype=torch.float32, device=dev), lm_state=torch.empty(B, N, dtype=torch.int32, device=dev),
               lm_n=torch.empty(B, N, dtype=torch.int32, device=dev), lm_att=torch.empty(B, N, dtype=torch.float32, device=dev))
    check(_lib.load().m3_aed_ngram_result(C.byref(desc), _p(state), _nbytes(state), _p(lstate), _nbytes(lstate), _p(out["lm"]),
                                       _p(out["lm_state"]), _p(out["lm_n"]), _p(out["lm_att"]), _stream()), "m3_aed_ngram_result")
    return out


# ---- hotword biasing in that search (m3_aed_bias_*)
def aed_bias_desc(search_desc, pre_beam, max_frames=0):
    """The descriptor of the biased search: m3_aed_joint_desc; max_frames = 0 where there is no CTC part (ctc_weight = 0).
    Raises M3Error on what the library rejects."""
    return _aed_fused_desc(search_desc, pre_beam, max_frames, "m3_aed_bias_state_size")


def aed_bias_state_size(desc):
    return _lib.load().m3_aed_bias_state_size(C.byref(desc))


def aed_bias_scratch_size(desc):
    return _lib.load().m3_aed_bias_scratch_size(C.byref(desc))


def aed_bias_record(image, graph_of, cstate, cscratch):
    """m3_aed_bias: the device context image (int32 words), graph_of (B,) int32 on the device (either may be None where the call
    does not read it), the context state and scratch (uint8 blobs)"""
    img, nbytes = _image(image)
    b = _lib.AedBias()
    b.image, b.image_bytes = (img.value if img is not None else None), nbytes
    b.graph_of = graph_of.data_ptr() if graph_of is not None else None
    if graph_of is not None:
        assert graph_of.is_cuda and graph_of.dtype == torch.int32 and graph_of.is_contiguous()
    b.state, b.state_bytes = (cstate.data_ptr(), _nbytes(cstate)) if cstate is not None else (None, 0)
    b.scratch, b.scratch_bytes = (cscratch.data_ptr(), _nbytes(cscratch)) if cscratch is not None else (None, 0)
    return b


def aed_bias_reset(desc, bias):
    """after aed_search_reset (and the joint / LM resets): every slot in state 0 with bonus 0.0; refuses an image of another V"""
    check(_lib.load().m3_aed_bias_reset(C.byref(desc), C.byref(bias), _stream()), "m3_aed_bias_reset")


def aed_bias_score(desc, state, jstate, scratch, lstate, lscratch, logits, ctc, ctc_weight, lm_image, lm_on, alpha, beta, use_eos, bias):
    """aed_lm_score with every candidate's context arc and the biased key; lm_image / lm_on / lstate / lscratch None exactly when
    there is no LM, ctc / jstate / scratch None exactly when ctc_weight = 0"""
    assert tuple(logits.shape) == (desc.search.B * desc.search.beam, desc.search.V)
    assert lm_on is None or lm_on.numel() == desc.search.B
    check(_lib.load().m3_aed_bias_score(C.byref(desc), *_blobs(state, jstate, scratch, lstate, lscratch), *_rows(logits), *_opt_rows(ctc),
                                        float(ctc_weight), *_image(lm_image), _i32(lm_on), float(alpha), float(beta), int(bool(use_eos)),
                                        C.byref(bias), _stream()), "m3_aed_bias_score")


def aed_bias_prune(desc, state, jstate, scratch, lstate, lscratch, bias, done=None):
    """aed_lm_prune, the survivors' context state copied from the context scratch; jstate / scratch None: no CTC; lstate / lscratch
    None: no LM"""
    assert done is None or done.numel() == desc.search.B
    check(_lib.load().m3_aed_bias_prune(C.byref(desc), *_blobs(state, jstate, scratch, lstate, lscratch), C.byref(bias), _i32(done),
                                        _stream()), "m3_aed_bias_prune")


def aed_bias_result(desc, state, bias):
    """-> dict(bonus (B, beam) float32, ctx_state (B, beam) int32, ctx_att (B, beam) float32) on the device"""
    B, N, dev = desc.search.B, desc.search.beam, state.device
    out = dict(bonus=torch.empty(B, N, dtype=torch.float32, device=dev), ctx_state=torch.empty(B, N, dtype=torch.int32, device=dev),
               ctx_att=torch.empty(B, N, dtype=torch.float32, device=dev))
    check(_lib.load().m3_aed_bias_result(C.byref(desc), _p(state), _nbytes(state), C.byref(bias), _p(out["bonus"]), _p(out["ctx_state"]),
                                         _p(out["ctx_att"]), _stream()), "m3_aed_bias_result")
    return out


# ---------------------------------------------------------------------------------------- streaming operators
def cat_split_cache(in_cache, inp):
    """CatSplitCache plugin: (output (B, cache+input), out_cache (B, cache)); f32 or i32 rows."""
    lib = _lib.load()
    assert in_cache.dtype == inp.dtype and in_cache.element_size() == 4
    B, cd = in_cache.shape
    idim = inp.shape[1]
    assert inp.shape[0] == B
    out = torch.empty(B, cd + idim, dtype=inp.dtype, device=inp.device)
    out_cache = torch.empty(B, cd, dtype=inp.dtype, device=inp.device)
    check(lib.m3_cat_split_cache(_p(in_cache), _p(inp), B, cd, idim, _p(out), _p(out_cache), _stream()), "m3_cat_split_cache")
    return out, out_cache


def att_stream_softmax(scores, decode_frame_num, mask_idx, cache_len, scale):
    """AttStreamSoftmax plugin on scores (B, N, ld) (any leading split of N, e.g. (B, h, T, ld))."""
    lib = _lib.load()
    B, ld = scores.shape[0], scores.shape[-1]
    N = scores.numel() // max(B * ld, 1)
    out = torch.empty_like(scores)
    check(lib.m3_att_stream_softmax(_f32(scores), _i32(decode_frame_num), _i32(mask_idx), B, N, ld, int(cache_len),
                                    float(scale), _p(out), _stream()), "m3_att_stream_softmax")
    return out


def rel_positional_encoding(x, pe, scale, frame_num=None, max_offset=0):
    """RelPositionalEncoding plugin: (x * scale, pe[off:off+T] (1,T,D)[, frame_num + T]); off = frame_num[0] or 0."""
    lib = _lib.load()
    B, T, D = x.shape
    pe2 = pe.reshape(-1, D)
    y = torch.empty_like(x)
    pos = torch.empty(1, T, D, dtype=torch.float32, device=x.device)
    fn_out = None if frame_num is None else torch.empty_like(frame_num)
    check(lib.m3_rel_positional_encoding(_f32(x), _f32(pe2), pe2.shape[0], _i32(frame_num), int(max_offset), float(scale),
                                         B, T, D, _p(y), _p(pos), _p(fn_out), _stream()), "m3_rel_positional_encoding")
    return (y, pos) if frame_num is None else (y, pos, fn_out)


def _conv2d_desc(x, w, bias, act=_lib.ACT_RELU, out=None):
    B, T1, F1, Cc = x.shape
    if out is None:
        out = torch.empty(B, (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1, Cc, dtype=torch.float32, device=x.device)
    d = _lib.Conv2dDesc()
    d.inp, d.w, d.bias, d.out = _f32(x).value, _f32(w).value, (_f32(bias).value if bias is not None else None), _f32(out).value
    d.B, d.T1, d.F1, d.C, d.act = B, T1, F1, Cc, int(act)
    return d, out


def conv2d_workspace_size(B, T1, F1, Cc, act=_lib.ACT_RELU):
    """bytes of split-K scratch subsample_conv2_ws takes for this shape (m3_conv2d_3x3s2_workspace_size); 0: no split-K problem"""
    return _lib.load().m3_conv2d_3x3s2_workspace_size(B, T1, F1, Cc, int(act))


def subsample_conv2_ws(x, w, bias, workspace, act=_lib.ACT_RELU, out=None):
    """subsample_conv2 with a caller-owned uint8 workspace (m3_conv2d_3x3s2_ws): split-K where the shape takes it"""
    d, out = _conv2d_desc(x, w, bias, act, out)
    check(_lib.load().m3_conv2d_3x3s2_ws(d.inp, d.w, d.bias, d.B, d.T1, d.F1, d.C, d.act, d.out, _p(workspace),
                                         workspace.numel() if workspace is not None else 0, _stream()), "m3_conv2d_3x3s2_ws")
    return out


def subsample_conv2_ws_pair(a, ws_a, b, ws_b, which=3):
    """two split-K implicit convs in one GEMM launch and one reduce launch (m3_conv2d_3x3s2_ws_pair).  Keys of a / b: x, w, bias
    and optionally act, out."""
    (da, oa), (db, ob) = _conv2d_desc(**a), _conv2d_desc(**b)
    check(_lib.load().m3_conv2d_3x3s2_ws_pair(C.byref(da), _p(ws_a), ws_a.numel(), C.byref(db), _p(ws_b), ws_b.numel(), int(which),
                                              _stream()), "m3_conv2d_3x3s2_ws_pair")
    return oa, ob


def subsample_conv2(x, w, bias, act=_lib.ACT_RELU):
    """Conv2d(C, C, 3, stride 2) on channel-last (B,T1,F1,C) as implicit GEMM; act = ACT_RELU (fused, default) or ACT_NONE."""
    lib = _lib.load()
    B, T1, F1, Cc = x.shape
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    out = torch.empty(B, T2, F2, Cc, dtype=torch.float32, device=x.device)
    check(lib.m3_conv2d_3x3s2(_f32(x), _f32(w), _f32(bias), B, T1, F1, Cc, int(act), _p(out), _stream()),
          "m3_conv2d_3x3s2")
    return out


# ---- the packed-row and bf16-row operand forms (include/m3asr.h "Packed rows")
def pack_plan(lens, T, feat_len=None, row0=None, pad_of=None):
    """row plan of a ragged batch (m3_pack_plan): lens (B,) int32 -> row0 (B + 1,), pad_of (B * T,).  feat_len (B,) int32: lens is
    an output too (the subsampled lengths)."""
    B = lens.numel()
    row0 = row0 if row0 is not None else torch.empty(B + 1, dtype=torch.int32, device=lens.device)
    pad_of = pad_of if pad_of is not None else torch.empty(B * T, dtype=torch.int32, device=lens.device)
    assert row0.numel() == B + 1 and pad_of.numel() == B * T and (feat_len is None or feat_len.numel() == B)
    check(_lib.load().m3_pack_plan(_i32(lens), B, T, _i32(row0), _i32(pad_of), _i32(feat_len), _stream()), "m3_pack_plan")
    return row0, pad_of


def unpack_rows(rows, row0, B, T, out=None):
    """padded (B * T, n) <- packed rows (P, n) (m3_unpack_rows): zeros behind every utterance's last frame"""
    n = rows.shape[1]
    if out is None:
        out = torch.empty(B * T, n, dtype=torch.float32, device=rows.device)
    assert tuple(out.shape) == (B * T, n) and row0.numel() == B + 1
    check(_lib.load().m3_unpack_rows(_f32(rows), _i32(row0), B, T, n, _f32(out), _stream()), "m3_unpack_rows")
    return out


def conv2d_kernel(B, T1, F1, Cc, act=_lib.ACT_RELU, w_bf16=False, with_workspace=False):
    """name of the device kernel the 3x3 / stride-2 conv runs for a shape (host-only query, m3_conv2d_3x3s2_kernel); None if refused"""
    name = _lib.load().m3_conv2d_3x3s2_kernel(B, T1, F1, Cc, int(act), int(bool(w_bf16)), int(bool(with_workspace)))
    return name.decode() if name else None


def conv2d_frames(x, w, bias, frames=None, act=_lib.ACT_RELU, out=None):
    """subsample_conv2 with the valid output frames per utterance on the device (m3_conv2d_3x3s2_frames); w fp32 or bf16"""
    B, T1, F1, Cc = x.shape
    if out is None:
        out = torch.empty(B, (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1, Cc, dtype=torch.float32, device=x.device)
    assert w.dtype in (torch.float32, torch.bfloat16)
    check(_lib.load().m3_conv2d_3x3s2_frames(_f32(x), _p(w), _f32(bias), B, T1, F1, Cc, int(act), _i32(frames),
                                             int(w.dtype == torch.bfloat16), _f32(out), _stream()), "m3_conv2d_3x3s2_frames")
    return out


def relpos_attention_packed(qkv, p, pos_u, pos_v, lens, B, T, H, dk, out, row0=None, chunk=0, left_chunks=-1):
    """the attention core on packed rows (m3_relpos_attention_packed; m3_relpos_attention_bf16_packed for a bf16 qkv): qkv
    (rows, 3 * H * dk) and out (rows, H * dk) hold the packed rows of the plan row0 (None: the B * T padded rows); a bf16 out on
    fp32 rows asks for the rounded copy (out_bf16)."""
    lib = _lib.load()
    D = H * dk
    assert qkv.shape[1] == 3 * D and out.shape[1] == D and p.shape[1] == D and p.shape[0] >= T
    d = _lib.AttentionDesc()
    (d.qkv, d.ldq), (d.p, d.ldp), (d.out, d.ldo) = [(q.value, ld) for q, ld in (_rows(qkv, qkv.dtype), _rows(p), _rows(out, out.dtype))]
    d.pos_u, d.pos_v, d.len = _f32(pos_u).value, _f32(pos_v).value, (_i32(lens).value if lens is not None else None)
    d.B, d.T, d.H, d.dk, d.scale, d.chunk, d.left_chunks = B, T, H, dk, 1.0 / math.sqrt(dk), int(chunk), int(left_chunks)
    if qkv.dtype == torch.bfloat16:
        assert out.dtype == torch.bfloat16
        check(lib.m3_relpos_attention_bf16_packed(C.byref(d), _i32(row0), _stream()), "m3_relpos_attention_bf16_packed")
    else:
        check(lib.m3_relpos_attention_packed(C.byref(d), _i32(row0), int(out.dtype == torch.bfloat16), _stream()), "m3_relpos_attention_packed")
    return out


def dwconv_ln_silu_packed(z, w_kc, bias, gamma, beta, eps, B, T, out, plan=None, left_fill=None, glu=False, gate_sigmoided=False):
    """the depthwise conv on packed rows (m3_dwconv_ln_silu_packed).  plan = (pad_of, row0, lens) of pack_plan, None: the padded
    layout.  z: the packed rows and the pad row behind them; glu: value | gate rows (may be row-strided).  out (rows, D) fp32, or
    bf16 for the rounded result."""
    K, D = w_kc.shape
    d = _lib.DwconvDesc()
    if glu:
        assert z.shape[1] == 2 * D
        zp, d.ldz = _rows(z)
        d.z = zp.value
    else:
        d.z = _f32(z).value
    d.gate_sigmoided = int(bool(gate_sigmoided))
    d.w_kc, d.bias, d.out = _f32(w_kc).value, _f32(bias).value, _p(out).value
    d.gamma, d.beta = (_f32(gamma).value if gamma is not None else None), (_f32(beta).value if beta is not None else None)
    d.left_fill = _f32(left_fill).value if left_fill is not None else None
    d.eps, d.B, d.T, d.D, d.K = float(eps), B, T, D, K
    pad_of, row0, lens = plan if plan is not None else (None, None, None)
    check(_lib.load().m3_dwconv_ln_silu_packed(C.byref(d), _i32(pad_of), _i32(row0), _i32(lens), int(out.dtype == torch.bfloat16), _stream()),
          "m3_dwconv_ln_silu_packed")
    return out


def layer_norm_ex(x, gamma, beta, eps, y=None, y_bf16=None, y_stats=None, ln2=None, y2=None):
    """layer_norm with its side results (m3_layer_norm_ex): y_bf16 the rounded copy, y_stats (rows, 4, 2) its row statistics,
    ln2 = (gamma2, beta2, eps2) with y2 = LN2(y).  y may be x."""
    D = x.shape[-1]
    y = y if y is not None else torch.empty_like(x)
    g2, b2, e2 = ln2 if ln2 is not None else (None, None, 0.0)
    check(_lib.load().m3_layer_norm_ex(_f32(x), _f32(gamma), _f32(beta), float(eps), _f32(y), x.numel() // D, D, _p(y_bf16), _f32(y_stats),
                                       _f32(g2), _f32(b2), float(e2), _f32(y2), _stream()), "m3_layer_norm_ex")
    return y


def row_stats_bf16(xb, stats=None):
    """(sum, sum of squares) of every row of a dense bf16 matrix -> (rows, 4, 2), total in part 0 (m3_row_stats_bf16)"""
    rows, D = xb.shape
    assert xb.dtype == torch.bfloat16
    stats = stats if stats is not None else torch.empty(rows, 4, 2, dtype=torch.float32, device=xb.device)
    check(_lib.load().m3_row_stats_bf16(_p(xb), rows, D, _f32(stats), _stream()), "m3_row_stats_bf16")
    return stats


def rows_to_bf16(x, out=None):
    """dense bf16 copy of the fp32 rows x (may be a row-strided view) (m3_rows_to_bf16)"""
    S, D = x.shape
    out = out if out is not None else torch.empty(S, D, dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (S, D)
    xp, ldx = _rows(x)
    check(_lib.load().m3_rows_to_bf16(xp, ldx, S, D, _p(out), _stream()), "m3_rows_to_bf16")
    return out


# ---------------------------------------------------------------------------------------- small plugins
def att_masked_softmax(scores, lens, scale):
    lib = _lib.load()
    B, H, T1, T2 = scores.shape
    out = torch.empty_like(scores)
    check(lib.m3_att_masked_softmax(_f32(scores), _i32(lens), B, H, T1, T2, float(scale), _p(out), _stream()),
          "m3_att_masked_softmax")
    return out


def masked_fill(x, lens, fill):
    lib = _lib.load()
    B, Cc, T = x.shape
    y = torch.empty_like(x)
    check(lib.m3_masked_fill(_f32(x), _i32(lens), B, Cc, T, float(fill), _p(y), _stream()), "m3_masked_fill")
    return y


def glu(x, dim):
    lib = _lib.load()
    dim = dim % x.dim()
    outer = int(math.prod(x.shape[:dim]))
    inner = int(math.prod(x.shape[dim + 1:]))
    Cc = x.shape[dim] // 2
    shape = list(x.shape)
    shape[dim] = Cc
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    check(lib.m3_glu(_f32(x), outer, Cc, inner, _p(y), _stream()), "m3_glu")
    return y


def mask_conv2d_sample(lens, left_padding, stride):
    lib = _lib.load()
    out = torch.empty_like(lens)
    check(lib.m3_mask_conv2d_sample(_i32(lens), lens.numel(), left_padding, stride, _p(out), _stream()),
          "m3_mask_conv2d_sample")
    return out


def scale(x, s):
    lib = _lib.load()
    y = torch.empty_like(x)
    check(lib.m3_scale(_f32(x), float(s), _p(y), x.numel(), _stream()), "m3_scale")
    return y


def unary(x, act):
    lib = _lib.load()
    y = torch.empty_like(x)
    check(lib.m3_unary(_f32(x), _p(y), x.numel(), act, _stream()), "m3_unary")
    return y


def binary(a, b, op):
    """Broadcasting element-wise sum / prod (TensorRT ElementWise semantics: equal rank, dims 1 broadcast)."""
    lib = _lib.load()
    assert a.dim() == b.dim(), "elementwise operands must have equal rank"
    shape = [max(x, y) for x, y in zip(a.shape, b.shape)]
    nd = len(shape)

    def strides(t):
        return [0 if t.shape[i] == 1 and shape[i] != 1 else t.stride(i) for i in range(nd)]

    y = torch.empty(shape, dtype=torch.float32, device=a.device)
    arr = C.c_int64 * nd
    check(lib.m3_binary(_f32(a), _f32(b), _p(y), arr(*shape), arr(*strides(a)), arr(*strides(b)), nd, op, _stream()),
          "m3_binary")
    return y


def permute_copy(x, perm):
    """Materialised permutation (TensorRT shuffle's transpose); x may be any strided view."""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32
    nd = x.dim()
    out_shape = [x.shape[p] for p in perm]
    in_strides = [x.stride(p) for p in perm]
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    arr = C.c_int64 * nd
    check(lib.m3_permute(C.c_void_p(x.data_ptr()), _p(y), arr(*out_shape), arr(*in_strides), nd, _stream()), "m3_permute")
    return y


def concat_last(a, b):
    lib = _lib.load()
    da, db = a.shape[-1], b.shape[-1]
    rows = a.numel() // da
    y = torch.empty(tuple(a.shape[:-1]) + (da + db,), dtype=torch.float32, device=a.device)
    check(lib.m3_concat_last(_f32(a), da, _f32(b), db, _p(y), rows, _stream()), "m3_concat_last")
    return y


def softmax_lastdim(x):
    lib = _lib.load()
    n = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.m3_softmax(_f32(x), _p(y), x.numel() // n, n, _stream()), "m3_softmax")
    return y


def batched_matmul(a, b, transpose_b=False):
    """a (..., M, K) @ b (..., K, N) (or b (..., N, K) transposed); leading dims equal or 1 in b/a."""
    lib = _lib.load()
    if b.dim() < a.dim():          # fewer leading dims: broadcast like torch.matmul
        b = b.reshape((1,) * (a.dim() - b.dim()) + tuple(b.shape))
    elif a.dim() < b.dim():
        a = a.reshape((1,) * (b.dim() - a.dim()) + tuple(a.shape))
    M, K = a.shape[-2:]
    N = b.shape[-2] if transpose_b else b.shape[-1]
    lead = [max(x, y) for x, y in zip(a.shape[:-2], b.shape[:-2])]
    batch = int(math.prod(lead)) if lead else 1
    na, nb = int(math.prod(a.shape[:-2])), int(math.prod(b.shape[:-2]))
    if na not in (1, batch):      # partial broadcast (e.g. (1,h,..) against (B,h,..)): materialise with the copy kernel
        a = permute_copy(a.expand(tuple(lead) + tuple(a.shape[-2:])), tuple(range(a.dim())))
        na = batch
    if nb not in (1, batch):
        b = permute_copy(b.expand(tuple(lead) + tuple(b.shape[-2:])), tuple(range(b.dim())))
        nb = batch
    c = torch.empty(tuple(lead) + (M, N), dtype=torch.float32, device=a.device)
    sa = 0 if na == 1 and batch > 1 else M * K
    sb = 0 if nb == 1 and batch > 1 else b.shape[-2] * b.shape[-1]
    check(lib.m3_batched_matmul(_f32(a), _f32(b), _p(c), batch, M, N, K, sa, sb, int(transpose_b), _stream()),
          "m3_batched_matmul")
    return c


def depthwise_conv1d(x, w, bias, pad):
    lib = _lib.load()
    B, Cc, T = x.shape
    K = w.shape[-1]
    y = torch.empty(B, Cc, T + 2 * int(pad) - K + 1, dtype=torch.float32, device=x.device)
    check(lib.m3_depthwise_conv1d(_f32(x), _f32(w.reshape(Cc, K)), _f32(bias), B, Cc, T, K, pad, _p(y), _stream()),
          "m3_depthwise_conv1d")
    return y


def pad2d(x, pre, post):
    """TensorRT IPaddingLayer on the last two dims: pre = (h, w), post = (h, w) zeros."""
    lib = _lib.load()
    H, W = x.shape[-2], x.shape[-1]
    outer = x.numel() // max(H * W, 1)
    y = torch.empty(tuple(x.shape[:-2]) + (H + pre[0] + post[0], W + pre[1] + post[1]), dtype=torch.float32, device=x.device)
    check(lib.m3_pad2d(_f32(x), outer, H, W, int(pre[0]), int(post[0]), int(pre[1]), int(post[1]), _p(y), _stream()), "m3_pad2d")
    return y
