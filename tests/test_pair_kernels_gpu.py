"""The six paired-launch (dual) kernels of the B = 1 fp32 engine, called directly through the pair entries of the C ABI
(include/m3asr.h "paired launches") on two UNEQUAL problems:

  gemm_f32_dual_kernel          m3_linear_pair             splitk_reduce_dual_kernel     (the reduce launch of both split-K pairs)
  gemm_f32_splitk_dual_kernel   m3_linear_ws_pair, m3_conv2d_3x3s2_ws_pair (the implicit-conv instantiation)
  relpos_attention_dual_kernel  m3_relpos_attention_pair   dwconv_ln_silu_dual_kernel    m3_dwconv_ln_silu_pair
  conv1_relu_dual_kernel        m3_subsample_conv1_pair

Every case makes three assertions, for the pair (a, b) and for the swapped pair (b, a):
  bits    each half of the paired launch equals the single ABI call on the same operands bit for bit (guarded.same_bits);
  value   each half is within the single operator's bound (tests/test_kernels_gpu.py) of a float64 torch reference, per element:
          2e-5 / 2e-5 linear and depthwise conv, 3e-5 / 3e-5 split-K, conv2 and attention, 1e-5 / 1e-5 conv1;
  guards  operands sit in tests/guarded.py buffers (row-strided wherever the ABI has a stride, NaN around every input); after
          every launch every output's guard holds its pattern and no element of the output view still holds it.

Tile and split counts are worked out here from the rules of skinny_grid and splitk_ranges (csrc/gemm_plan.hip) and asserted
where a count is the point of a case: the second problem's work-group ids start at the first problem's count rounded up to a
multiple of 8.

Not reachable at the boundary, so not refused here: a split-K pair of an implicit conv with a plain problem (each pair entry
takes two problems of one kind).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded as G
from m3asr import ops, _lib
from m3asr._lib import M3Error
from m3asr.plan import fold_layernorm
from stream_kernels_ref import attention_ref

ERRS = {}      # operator -> largest |error| against the float64 reference seen in this run (printed per case)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return None if t is None else t.cuda().contiguous()


def close(got, want, rtol, atol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    op = what.split(":")[0]
    ERRS[op] = max(ERRS.get(op, 0.0), float(err.max()))
    print("%s max abs err %.3e (max |ref| %.3e, bound %.1e / %.1e; largest so far for %s: %.3e)" % (
        what, float(err.max()), float(want.abs().max()), rtol, atol, op, ERRS[op]))
    assert bool((err <= bound).all()), "%s max abs err %.3e (max |ref| %.3e), worst excess %.3e" % (
        what, float(err.max()), float(want.abs().max()), float((err - bound).max()))


def cdiv(a, b):
    return -(-a // b)


def align8(n):
    return cdiv(n, 8) * 8


class Prob:
    """one problem of a launch: the keyword arguments of its wrapper, its guarded outputs, the float64 reference of the main
    output (`valid`: the rows it is compared on; None: all) and the bound"""

    def __init__(self, kw, out, want, tol, valid=None, extra_outs=(), name=""):
        self.kw, self.out, self.want, self.tol, self.valid, self.extra_outs, self.name = kw, out, want, tol, valid, list(extra_outs), name

    @property
    def ws(self):
        """the split-K workspace (the first extra output) as the uint8 tensor the wrappers take"""
        return self.extra_outs[0].view.view(torch.uint8)

    def check(self, what):
        for i, o in enumerate([self.out] + self.extra_outs):
            o.check("%s %s output %d" % (what, self.name, i))
            assert not bool(o.untouched().any()), "%s %s output %d: %d element(s) never written" % (
                what, self.name, i, int(o.untouched().sum()))
        got, want = self.out.view.reshape(self.want.shape), self.want
        if self.valid is not None:
            got, want = got[self.valid], want[self.valid]
        close(got, want, self.tol, self.tol, "%s: %s %s" % (self.name.split(" ")[0], what, self.name))


def run_pair_case(mk_a, mk_b, single, pair):
    """mk_a / mk_b: factories of fresh Prob objects (fresh output buffers, the same inputs); single(p) and pair(p, q) launch"""
    ref = []
    for mk in (mk_a, mk_b):
        p = mk()
        single(p)
        torch.cuda.synchronize()
        p.check("single")
        ref.append(p)
    for order in ((0, 1), (1, 0)):
        ps = [(mk_a, mk_b)[i]() for i in order]
        pair(ps[0], ps[1])
        torch.cuda.synchronize()
        for i, p in zip(order, ps):
            p.check("pair%s" % (order,))
            for o, r in zip([p.out] + p.extra_outs, [ref[i].out] + ref[i].extra_outs):
                assert G.same_bits(o.view, r.view), "pair %s: %s differs from the single launch (max abs diff %g)" % (
                    order, p.name, float((o.view.double() - r.view.double()).abs().max()))


# ================================================================================================ GEMM pair
def skinny_tiles(M, n_out):
    """(column tiles, row tiles) of a skinny fp32 problem with 16-row tiles (skinny_grid with mt = 1: M <= 128)"""
    assert M <= 128
    return cdiv(n_out, 16), cdiv(M, 16)


def gemm_problem(M, N, K, *, act=_lib.ACT_NONE, bias=True, alpha=1.0, resid=None, lens=None, rpb=0, mask_in=False, mask_out=False,
                 folded=False, seed=0, tol=2e-5):
    """factory of one m3_linear problem on guarded operands.  resid: None / "strided" (own buffer, ldr != ldy) / "inplace"."""
    glu = act == _lib.ACT_GLU
    n_out = N // 2 if glu else N
    a = rnd(M, K, seed=seed + 1)
    w, b = rnd(N, K, seed=seed + 2, scale=K ** -0.5), (rnd(N, seed=seed + 3) if bias else None)
    res = rnd(M, n_out, seed=seed + 4) if resid else None
    pad = None
    if lens is not None:
        L = torch.tensor(lens, dtype=torch.int32)
        pad = (torch.arange(rpb).view(1, rpb) >= L.view(-1, 1)).reshape(M, 1)
    kw = dict(act=act, alpha=alpha)
    a64, w64 = a.double(), w.double()
    b64 = b.double() if bias else torch.zeros(N, dtype=torch.float64)
    if folded:
        ga, be = rnd(K, seed=seed + 5) * 0.2 + 1.0, rnd(K, seed=seed + 6, scale=0.1)
        f = fold_layernorm(w, b if bias else torch.zeros(N), ga, be)
        x = F.layer_norm(a64, (K,), ga.double(), be.double(), 1e-12)
        if mask_in:
            x = x.masked_fill(pad, 0.0)
        z = x @ w64.t() + b64
        w_dev, b_dev = dev(f["ln.weight"]), dev(f["ln.bias"])
        kw["ln_folded"] = (dev(f["ln.wsum"]), dev(f["ln.wbeta"]) if mask_in else None, 1e-12)
    else:
        z = (a64.masked_fill(pad, 0.0) if mask_in else a64) @ w64.t() + b64
        w_dev, b_dev = dev(w), dev(b)
    if glu:
        z = z[:, :n_out] * torch.sigmoid(z[:, n_out:])
    z = {_lib.ACT_RELU: F.relu, _lib.ACT_SILU: F.silu}.get(act, lambda t: t)(z)
    if mask_out:
        z = z.masked_fill(pad, 0.0)
    want = alpha * z + (res.double() if resid else 0.0)
    if lens is not None:
        kw.update(lens=dev(L), rows_per_batch=rpb, mask_in=mask_in, mask_out=mask_out)
    ga_ = G.strided_in(a)
    gr = G.strided_in(res, ld=n_out + 12) if resid == "strided" else None
    name = "linear %dx%dx%d" % (M, N, K)

    def make():
        gy = G.strided_out(M, n_out)
        k = dict(kw, a=ga_.view, w=w_dev, bias=b_dev, out=gy.view)
        if resid == "strided":
            assert gr.ld != gy.ld
            k["resid"] = gr.view
        elif resid == "inplace":
            gy.view.copy_(res.cuda())           # the guard keeps its pattern, the view holds the residual
            k["resid"] = gy.view
        return Prob(k, gy, want, tol, name=name)
    return make


def _linear_single(p):
    k = dict(p.kw)
    ops.linear(k.pop("a"), k.pop("w"), **k)


def _linear_pair(p, q):
    assert ops.linear_pair_kernel(p.kw, q.kw) == "gemm_f32_dual_kernel", _lib.last_error()
    ops.linear_pair(p.kw, q.kw)


GEMM_CASES = {
    # 64 tiles (32 column tiles: the XCD swizzle is on) vs 6 tiles (3 column tiles: off)
    "tiles64_vs_6": (dict(M=24, N=512, K=256, act=_lib.ACT_SILU), dict(M=17, N=48, K=512, bias=False, alpha=0.5, resid="strided"), (64, 6)),
    # 10 tiles: the second problem's work-groups start at 16 behind 6 idle ones; one row
    "idle_gap": (dict(M=17, N=80, K=64, bias=False), dict(M=1, N=1024, K=64), (10, 64)),
    # 8 waves (K = 1024), a partial column tile (24 = 16 + 8 columns)
    "nw8_partial_tile": (dict(M=24, N=256, K=1024), dict(M=40, N=24, K=1024, act=_lib.ACT_RELU), (32, 6)),
    # GLU with the folded LayerNorm (ln_wbeta) and the input mask; two utterances of 17 rows in the second problem
    "glu_folded_mask_in": (dict(M=24, N=512, K=256, act=_lib.ACT_GLU, folded=True, lens=[24], rpb=24, mask_in=True),
                           dict(M=34, N=1024, K=512, act=_lib.ACT_GLU, folded=True, lens=[17, 9], rpb=17, mask_in=True), (32, 96)),
    # epilogue variants: the in-place residual update next to an output mask with a residual
    "inplace_vs_mask_out": (dict(M=24, N=64, K=128, alpha=0.5, resid="inplace"),
                            dict(M=34, N=48, K=256, lens=[17, 9], rpb=17, mask_out=True, resid="strided"), (8, 9)),
}


@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm_pair(case):
    ka, kb, tiles = GEMM_CASES[case]
    for k, want in zip((ka, kb), tiles):
        nt, mt = skinny_tiles(k["M"], k["N"] // 2 if k.get("act") == _lib.ACT_GLU else k["N"])
        assert nt * mt == want
    if case == "tiles64_vs_6":
        assert skinny_tiles(24, 512)[0] % 8 == 0 and skinny_tiles(17, 48)[0] % 8 != 0          # swizzle on / off
    if case == "idle_gap":
        assert align8(10) - 10 == 6
    run_pair_case(gemm_problem(seed=10, **ka), gemm_problem(seed=20, **kb), _linear_single, _linear_pair)


# ================================================================================================ split-K pair, plain
def splitk_splits(M, N, K):
    """K ranges of a split-K problem (splitk_ranges): ~512 work-groups over the 64 x 64 tiles, >= 4 k-steps of 64 each, evened out"""
    tiles, nsteps = cdiv(M, 64) * cdiv(N, 64), K // 64
    splits = min(512 // tiles, nsteps // 4)
    return cdiv(nsteps, cdiv(nsteps, splits))


def splitk_problem(M, N, K, *, act=_lib.ACT_NONE, alpha=1.0, seed=0):
    a, w, b = rnd(M, K, seed=seed + 1), rnd(N, K, seed=seed + 2, scale=K ** -0.5), rnd(N, seed=seed + 3)
    z = a.double() @ w.double().t() + b.double()
    want = alpha * {_lib.ACT_RELU: F.relu, _lib.ACT_SILU: F.silu}.get(act, lambda t: t)(z)
    ga_, w_dev, b_dev = G.strided_in(a), dev(w), dev(b)

    def make():
        gy = G.strided_out(M, N)
        k = dict(a=ga_.view, w=w_dev, bias=b_dev, out=gy.view, act=act, alpha=alpha)
        need = ops.linear_workspace_size(**k)
        assert need == splitk_splits(M, N, K) * 4 * M * N           # the planner's split count is the one worked out here
        ws = G.flat_out((need // 4,))          # fp32 guard: no partial sum equals the signalling-NaN pattern
        return Prob(k, gy, want, 3e-5, extra_outs=[ws], name="splitk %dx%dx%d" % (M, N, K))
    return make


def _splitk_single(p):
    k = dict(p.kw)
    ops.linear(k.pop("a"), k.pop("w"), split_k=True, workspace=p.ws, **k)


def _splitk_pair(p, q, which=3):
    assert ops.linear_pair_kernel(p.kw, q.kw, with_workspace=True) == "gemm_f32_splitk_dual_kernel", _lib.last_error()
    ops.linear_ws_pair(p.kw, p.ws, q.kw, q.ws, which)


def test_splitk_pair_plain():
    # 3 tiles x 14 ranges (66 k-steps in ranges of 5: the last holds one step) = 42 work-groups: the second problem starts at 48;
    # 1 tile x 16 ranges
    assert (splitk_splits(130, 64, 4224), splitk_splits(7, 64, 4096)) == (14, 16)
    assert cdiv(66, 14) == 5 and 66 - 13 * 5 == 1 and align8(3 * 14) == 48
    mk_a, mk_b = splitk_problem(130, 64, 4224, seed=30), splitk_problem(7, 64, 4096, act=_lib.ACT_SILU, alpha=0.5, seed=40)
    run_pair_case(mk_a, mk_b, _splitk_single, _splitk_pair)
    # the GEMM launch and the reduce launch apart (the engine's two stages), on fresh workspaces: the same bits as both at once
    for mks in ((mk_a, mk_b), (mk_b, mk_a)):
        both, apart = [mk() for mk in mks], [mk() for mk in mks]
        _splitk_pair(both[0], both[1], 3)
        _splitk_pair(apart[0], apart[1], 1)
        torch.cuda.synchronize()
        for p in apart:                                   # the GEMM launch writes partial tiles only
            p.extra_outs[0].check("GEMM launch workspace")
            assert not bool(p.extra_outs[0].untouched().all()) and bool(p.out.untouched().all())
        _splitk_pair(apart[0], apart[1], 2)
        torch.cuda.synchronize()
        for p, q in zip(both, apart):
            q.check("which 1 then 2")
            assert G.same_bits(p.out.view, q.out.view) and G.same_bits(p.extra_outs[0].view, q.extra_outs[0].view)


# ================================================================================================ split-K pair, implicit conv
def conv2_problem(T1, F1, Cc, act, seed):
    x = rnd(1, T1, F1, Cc, seed=seed + 1)
    w, b = rnd(Cc, Cc, 3, 3, seed=seed + 2, scale=(9 * Cc) ** -0.5), rnd(Cc, seed=seed + 3, scale=0.1)
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=2)
    want = (F.relu(y) if act == _lib.ACT_RELU else y).permute(0, 2, 3, 1).contiguous()
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    gx, w_dev, b_dev = G.flat_in(x), dev(w.permute(0, 2, 3, 1)), dev(b)
    need = ops.conv2d_workspace_size(1, T1, F1, Cc, act)
    # each single problem really takes the implicit-conv split-K kernel: a workspace of the size worked out here is asked for
    assert need == splitk_splits(T2 * F2, Cc, 9 * Cc) * 4 * T2 * F2 * Cc and need > 0

    def make():
        gy = G.flat_out((1, T2, F2, Cc))
        ws = G.flat_out((need // 4,))
        return Prob(dict(x=gx.view, w=w_dev, bias=b_dev, act=act, out=gy.view), gy, want, 3e-5, extra_outs=[ws],
                    name="conv2 %dx%dx%d" % (T1, F1, Cc))
    return make


def _conv2_single(p):
    k = p.kw
    ops.subsample_conv2_ws(k["x"], k["w"], k["bias"], p.ws, act=k["act"], out=k["out"])


def _conv2_pair(p, q):
    ops.subsample_conv2_ws_pair(p.kw, p.ws, q.kw, q.ws)


def test_splitk_pair_implicit_conv():
    # C = 512, (5, 5) -> 4 rows: 8 tiles x 18 ranges = 144 work-groups.  C = 576, (7, 9) -> 12 rows: 9 tiles, 81 k-steps in 17
    # ranges = 153 work-groups (the swapped pair's second problem starts at 160)
    assert (splitk_splits(4, 512, 4608), splitk_splits(12, 576, 5184)) == (18, 17) and 9 * 17 == 153 and align8(153) == 160
    run_pair_case(conv2_problem(5, 5, 512, _lib.ACT_RELU, 50), conv2_problem(7, 9, 576, _lib.ACT_NONE, 60), _conv2_single, _conv2_pair)


# ================================================================================================ attention pair
def att_problem(B, T, H, dk, lens, chunk=0, left=-1, seed=0):
    D = H * dk
    qkv, p = rnd(B * T, 3 * D, seed=seed + 1), rnd(T, D, seed=seed + 2)
    u, v = rnd(H, dk, seed=seed + 3, scale=0.3), rnd(H, dk, seed=seed + 4, scale=0.3)
    L = torch.tensor(lens, dtype=torch.int32)
    want = attention_ref(qkv, p, u, v, L, B, T, H, dk, chunk, left)
    valid = (torch.arange(T).view(1, T) < L.view(B, 1)).reshape(B * T)     # rows past len: against the single launch only
    gq, gp = G.strided_in(qkv), G.strided_in(p, ld=2 * D)
    u_d, v_d, L_d = dev(u), dev(v), dev(L)

    def make():
        go = G.strided_out(B * T, D)
        return Prob(dict(qkv=gq.view, p=gp.view, pos_u=u_d, pos_v=v_d, lens=L_d, B=B, T=T, H=H, dk=dk, chunk=chunk, left_chunks=left,
                         out=go.view), go, want, 3e-5, valid=valid, name="attention B%d T%d H%d dk%d" % (B, T, H, dk))
    return make


def _att_single(p):
    ops.relpos_attention(**p.kw)


def _att_pair(p, q):
    ops.relpos_attention_pair(p.kw, q.kw)


@pytest.mark.parametrize("dk_small,dk_batch", [(64, 64), (128, 128), (128, 64), (64, 128)])
def test_attention_pair(dk_small, dk_batch):
    """One utterance of 17 frames, 3 heads, chunk mask (chunk 4, one left chunk): 2 query tiles x 3 = 6 work-groups, no XCD map,
    2 idle work-groups before the second problem.  Two utterances of 24 frames ([24, 9] valid), 4 heads, no chunk mask: H B = 8,
    the XCD map is on.  Both orders run, so every (DK0, DK1) instantiation sees the small problem first and second."""
    assert cdiv(17, 16) * 3 * 1 == 6 and (3 * 1) % 8 != 0 and align8(6) - 6 == 2 and (4 * 2) % 8 == 0
    run_pair_case(att_problem(1, 17, 3, dk_small, [17], chunk=4, left=1, seed=70), att_problem(2, 24, 4, dk_batch, [24, 9], seed=80),
                  _att_single, _att_pair)


def test_attention_pair_one_frame():
    run_pair_case(att_problem(1, 1, 3, 128, [1], seed=90), att_problem(2, 24, 4, 64, [24, 9], chunk=4, left=1, seed=80), _att_single, _att_pair)


# ================================================================================================ depthwise pair
def dw_problem(B, T, D, K, *, ln=True, causal=False, glu=None, eps=1e-5, seed=0):
    """glu: None / "load" (value | gate rows, strided) / "sigmoided" (the gate columns hold sigmoid(gate), formed on the host in
    float64 and rounded to fp32)"""
    w_kc, b = rnd(K, D, seed=seed + 2, scale=K ** -0.5), rnd(D, seed=seed + 3, scale=0.1)
    ga, be = (rnd(D, seed=seed + 4) * 0.2 + 1.0, rnd(D, seed=seed + 5, scale=0.1)) if ln else (None, None)
    fill = rnd(D, seed=seed + 6) if causal else None
    if glu:
        vg = rnd(B * T, 2 * D, seed=seed + 1)
        if glu == "sigmoided":
            vg[:, D:] = torch.sigmoid(vg[:, D:].double()).float()
            z64 = vg[:, :D].double() * vg[:, D:].double()
        else:
            z64 = vg[:, :D].double() * torch.sigmoid(vg[:, D:].double())
        gz = G.strided_in(vg, ld=2 * D + 24)
        assert gz.ld > 2 * D
    else:
        z = rnd(B * T, D, seed=seed + 1)
        z64 = z.double()
        gz = G.flat_in(z)
    z64 = z64.view(B, T, D).transpose(1, 2)
    w64 = w_kc.double().t().unsqueeze(1)
    if causal:
        left = fill.double().view(1, D, 1).expand(B, D, K - 1)
        y = F.conv1d(torch.cat([left, z64], 2), w64, b.double(), groups=D)
    else:
        y = F.conv1d(z64, w64, b.double(), padding=(K - 1) // 2, groups=D)
    y = y.transpose(1, 2)
    if ln:
        y = F.layer_norm(y, (D,), ga.double(), be.double(), eps)
    want = (y * torch.sigmoid(y)).reshape(B * T, D)
    w_d, b_d, ga_d, be_d, fill_d = dev(w_kc), dev(b), dev(ga), dev(be), dev(fill)

    def make():
        go = G.flat_out((B * T, D))
        k = dict(z=gz.view, w_kc=w_d, bias=b_d, gamma=ga_d, beta=be_d, eps=eps, B=B, T=T, out=go.view)
        if causal:
            k["left_fill"] = fill_d
        if glu:
            k.update(glu=True, gate_sigmoided=glu == "sigmoided")
        return Prob(k, go, want, 2e-5, name="dwconv B%d T%d D%d K%d" % (B, T, D, K))
    return make


def _dw_single(p):
    k = p.kw
    args = (k["z"], k["w_kc"], k["bias"], k["gamma"], k["beta"], k["eps"])
    if k.get("glu"):
        assert not k["gate_sigmoided"]
        ops.dwconv_glu_ln_silu(*args, k["B"], k["T"], out=k["out"])
    elif "left_fill" in k:
        ops.dwconv_ln_silu_causal(*args, k["left_fill"], k["B"], k["T"], out=k["out"])
    else:
        ops.dwconv_ln_silu(*args, k["B"], k["T"], out=k["out"])


def _dw_pair(p, q):
    ops.dwconv_ln_silu_pair(p.kw, q.kw)


DW_CASES = {
    "symmetric_second_without_ln": (dict(D=64, K=15), dict(D=64, K=15, ln=False)),
    "symmetric_8_tap_template": (dict(D=32, K=31), dict(D=32, K=31, eps=1e-3)),
    "causal_k15": (dict(D=64, K=15, causal=True), dict(D=64, K=15, causal=True, eps=1e-3)),
    "causal_k8": (dict(D=64, K=8, causal=True), dict(D=64, K=8, causal=True, eps=1e-3)),
}


@pytest.mark.parametrize("case", list(DW_CASES))
def test_dwconv_pair(case):
    ka, kb = DW_CASES[case]
    run_pair_case(dw_problem(1, 5, seed=100, **ka), dw_problem(2, 9, seed=110, **kb), _dw_single, _dw_pair)


def test_dwconv_pair_glu_on_load():
    run_pair_case(dw_problem(1, 24, 256, 15, glu="load", seed=120), dw_problem(2, 17, 256, 15, glu="load", eps=1e-3, seed=130),
                  _dw_single, _dw_pair)


def test_dwconv_pair_gate_sigmoided():
    """The form whose gate columns hold sigmoid(gate) already has no single entry: bit identity with a single launch is NOT
    asserted here.  Each half is compared with the float64 reference on the gate values the kernel reads (sigmoid formed on the
    host in float64, rounded to fp32), in both orders, and the two orders must agree bit for bit."""
    mks = (dw_problem(1, 24, 256, 15, glu="sigmoided", seed=120), dw_problem(2, 17, 256, 15, glu="sigmoided", eps=1e-3, seed=130))
    outs = {}
    for order in ((0, 1), (1, 0)):
        ps = [mks[i]() for i in order]
        _dw_pair(ps[0], ps[1])
        torch.cuda.synchronize()
        for i, p in zip(order, ps):
            p.check("pair%s" % (order,))
            assert G.same_bits(outs.setdefault(i, p.out.view), p.out.view)


# ================================================================================================ conv1 pair
def conv1_problem(T, idim, Cc, *, relu, cmvn=False, seed=0):
    feat = torch.rand(1, T, idim, generator=torch.Generator().manual_seed(seed + 1))
    w0, b0 = rnd(Cc, 1, 3, 3, seed=seed + 2, scale=1 / 3), rnd(Cc, seed=seed + 3, scale=0.1)
    mean, istd = (rnd(idim, seed=seed + 4, scale=0.3) + 0.5, torch.rand(idim, generator=torch.Generator().manual_seed(seed + 5)) + 0.5)
    x = feat.double()
    if cmvn:
        x = (x - mean.double()) * istd.double()
    y = F.conv2d(x.unsqueeze(1), w0.double(), b0.double(), stride=2)
    want = (F.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()
    T1, F1 = (T - 3) // 2 + 1, (idim - 3) // 2 + 1
    gf, w_d, b_d = G.flat_in(feat), dev(w0.reshape(Cc, 9).t()), dev(b0)
    cm = (dev(mean), dev(istd)) if cmvn else None

    def make():
        go = G.flat_out((1, T1, F1, Cc))
        return Prob(dict(feat=gf.view, w9c=w_d, bias=b_d, act=_lib.ACT_RELU if relu else _lib.ACT_NONE, cmvn=cm, out=go.view), go, want, 1e-5,
                    name="conv1 T%d idim%d C%d" % (T, idim, Cc))
    return make


def _conv1_single(p):
    k = p.kw
    if k["cmvn"] is not None:
        assert k["act"] == _lib.ACT_RELU
        ops.subsample_conv1_cmvn(k["feat"], k["w9c"], k["bias"], k["cmvn"], out=k["out"])
    else:
        ops.subsample_conv1(k["feat"], k["w9c"], k["bias"], act=k["act"], out=k["out"])


@pytest.mark.parametrize("idim", [40, 9])
@pytest.mark.parametrize("C0,C1", [(32, 512), (512, 32), (1024, 4)])
def test_conv1_pair(idim, C0, C1):
    """B = 1, T = 13: 6 output rows, the second problem's rows start at 8; five column chunks: F1 = 19 in chunks of 4 (the last
    one holds 3) and F1 = 4 in chunks of 1 (the fifth is empty).  The work-group is sized by the larger channel count.  ReLU and
    CMVN on the first half, neither on the second; the first problem of each launch also forms the subsampled lengths."""
    T = 13
    T1, F1 = (T - 3) // 2 + 1, (idim - 3) // 2 + 1
    assert T1 == 6 and align8(T1) == 8 and (F1, cdiv(F1, 5), F1 - 4 * cdiv(F1, 5)) in ((19, 4, 3), (4, 1, 0))
    feat_len = torch.tensor([11], dtype=torch.int32)
    fl = dev(feat_len)
    lens = []

    def pair(p, q):
        lo = G.flat_out((1,), torch.int32)
        lens.append(lo)
        ops.subsample_conv1_pair(dict(p.kw, feat_len=fl, lens_out=lo.view), q.kw)

    run_pair_case(conv1_problem(T, idim, C0, relu=True, cmvn=True, seed=140), conv1_problem(T, idim, C1, relu=False, seed=150),
                  _conv1_single, pair)
    assert len(lens) == 2
    for lo in lens:
        lo.check("lens_out")
        assert lo.view.cpu().tolist() == [((11 - 3) // 2 + 1 - 3) // 2 + 1]


# ================================================================================================ refusals
def _refused(pair, p, q, text):
    with pytest.raises(M3Error) as e:
        pair(p, q)
    assert text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for r in (p, q):
        for o in [r.out] + r.extra_outs:
            o.check("refused pair")
            assert bool(o.untouched().all()), "a refused pair wrote to an output"


def test_gemm_pair_refusals():
    base = dict(M=24, N=512, K=512)
    pair = lambda p, q: ops.linear_pair(p.kw, q.kw)
    groups = "load groups: the paired kernel takes"
    cases = [
        (dict(M=24, N=512, K=1024), "differ in waves (4 / 8)"),
        (dict(M=24, N=512, K=512, act=_lib.ACT_GLU), "GLU (0 / 1)"),
        (dict(M=24, N=512, K=512, folded=True), "folded LayerNorm (0 / 1)"),
        (dict(M=200, N=1024, K=512), "32-row tiles"),
        (dict(M=24, N=512, K=528), "1 has 16-row tiles, 4 waves, 2 " + groups),
    ]
    for kb, text in cases:
        _refused(pair, gemm_problem(seed=10, **base)(), gemm_problem(seed=20, **kb)(), text)
        assert ops.linear_pair_kernel(gemm_problem(seed=10, **base)().kw, gemm_problem(seed=20, **kb)().kw) is None
    # forms gemm_problem does not build: the affine LayerNorm, concat operands, bf16 weights
    p, q = gemm_problem(seed=10, **base)(), gemm_problem(seed=20, **base)()
    q.kw["ln"] = (dev(torch.ones(512)), dev(torch.zeros(512)), 1e-5)
    _refused(pair, p, q, "1 has 16-row tiles, 4 waves, 1 load group: the paired kernel takes")
    p, q = gemm_problem(seed=10, **base)(), gemm_problem(seed=20, M=24, N=512, K=256)()
    q.kw["a2"] = G.strided_in(rnd(24, 256, seed=5)).view
    q.kw["w"] = dev(rnd(512, 512, seed=6))
    _refused(pair, p, q, "1 has 16-row tiles, 4 waves, 1 load group: the paired kernel takes")
    p, q = gemm_problem(seed=10, **base)(), gemm_problem(seed=20, **base)()
    q.kw["w"] = q.kw["w"].to(torch.bfloat16)
    _refused(pair, p, q, "problem 1 runs gemm_bf16w_kernel")
    # one output inside the other
    p, q = gemm_problem(seed=10, **base)(), gemm_problem(seed=20, M=8, N=512, K=512)()
    q.kw["out"] = p.kw["out"][8:16]
    _refused(pair, p, q, "the two outputs overlap")


def test_splitk_pair_refusals():
    p, q = splitk_problem(130, 64, 4224, seed=30)(), splitk_problem(7, 64, 4096, seed=40)()
    _refused(lambda p, q: ops.linear_ws_pair(p.kw, p.ws, q.kw, p.ws), p, q, "each problem needs its own workspace")
    p, q = splitk_problem(130, 64, 4224, seed=30)(), gemm_problem(seed=20, M=24, N=512, K=512)()
    q.extra_outs = [G.flat_out((4096,), torch.uint8)]
    _refused(lambda p, q: ops.linear_ws_pair(p.kw, p.ws, q.kw, q.ws), p, q, "problem 1 is no split-K problem")
    p, q = conv2_problem(5, 5, 512, _lib.ACT_RELU, 50)(), conv2_problem(7, 9, 576, _lib.ACT_NONE, 60)()
    _refused(lambda p, q: ops.subsample_conv2_ws_pair(p.kw, q.ws, q.kw, q.ws), p, q,
             "each problem needs its own workspace")


def test_attention_pair_refusals():
    p, q = att_problem(1, 17, 3, 64, [17], seed=70)(), att_problem(2, 24, 4, 32, [24, 9], seed=80)()
    _refused(_att_pair, p, q, "head widths 64 / 32")
    _refused(_att_pair, q, p, "head widths 32 / 64")


def test_dwconv_pair_refusals():
    a = dict(D=64, K=15)
    for kb, text in ((dict(D=32, K=15), "channels 64 / 32"), (dict(D=64, K=7), "taps 15 / 7"), (dict(D=64, K=15, causal=True), "causal 0 / 1")):
        _refused(_dw_pair, dw_problem(1, 5, seed=100, **a)(), dw_problem(2, 9, seed=110, **kb)(), text)


def test_conv1_pair_refusals():
    pair = lambda p, q: ops.subsample_conv1_pair(p.kw, q.kw)
    _refused(pair, conv1_problem(13, 9, 32, relu=True, seed=140)(), conv1_problem(15, 9, 32, relu=True, seed=150)(), "T 13 / 15")
    p, q = conv1_problem(13, 9, 32, relu=True, seed=140)(), conv1_problem(13, 9, 32, relu=False, seed=150)()
    q.kw["out"] = p.kw["out"]
    q.out = p.out
    _refused(pair, p, q, "the two outputs overlap")
