"""Entry points that had no direct test (m3_moe_combine / _bf16, m3_ep_send_map / m3_ep_recv_gate, m3_layer_norm beyond one
shape) against fp64 / the numpy statements of oracle/moe_index.py, and dense-ABI operators on guarded operands
(tests/guarded.py: NaN around every input, a bit pattern around every output that must survive the call)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded as G
from m3asr import ops, _lib
from m3asr._lib import M3Error
from oracle import encoder_ref as ref
from oracle.moe_index import moe_index_ref, local_scatter_ref, local_gather_ref, ep_send_map_ref, ep_recv_gate_ref

U = 2.0 ** -24          # unit roundoff of fp32


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.cuda().contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================================================ m3_moe_combine
def _mapping(kind, S, seed):
    rng = np.random.default_rng(seed)
    if kind == "identity":
        m = np.arange(S)
    elif kind == "permutation":
        m = rng.permutation(S)
    elif kind == "dropped":                       # about a third of the rows dropped; the others a permutation of [0, kept)
        keep = rng.random(S) < 0.67
        m = np.full(S, -1)
        m[keep] = rng.permutation(int(keep.sum()))
    else:
        m = np.full(S, -1)
    return torch.from_numpy(m.astype(np.int32))


COMBINE_D = [4, 252, 256, 260, 512, 1024, 1028, 2048]      # both sides of every NV switch of launch_moe_combine (256 / 512 / 1024)
COMBINE_S = [1, 3, 4, 5, 1090, 4097]                        # 4 rows per work-group: one below / at / above, long batches


@pytest.mark.parametrize("S", COMBINE_S)
@pytest.mark.parametrize("D", COMBINE_D)
def test_moe_combine_against_fp64(D, S):
    """out[s] = LN(resid[s] + alpha * gate[s] * rows[mapping[s]]), rows with mapping < 0 contribute 0.
    Without LayerNorm the kernel rounds three times per element: t = fl(alpha * gate), p = fl(t * row), out = fl(p + resid), so
    |out - exact| <= 2u |p| + u (|p| + |resid|) + O(u^2) <= 3u (|term| + |resid|), u = 2^-24; asserted at 4u (|term| + |resid|)
    (no absolute slack: a row that contributes 0 must give resid, or 0, exactly).  With LayerNorm: the 1e-5 / 1e-5 that
    test_linear_layernorm_prologue holds for m3_layer_norm, on unit-scale inputs.
    Every combination of gate_value / resid / ln present or NULL (8) x alpha in {1, 0.5} x four mappings, at every (D, S).
    out_bf16 must be out.to(bfloat16) bit for bit, and m3_moe_combine_bf16 with out_bf16 = NULL must give the same out."""
    n_rows = S + 3
    rows, res = rnd(n_rows, D, seed=1), rnd(S, D, seed=2)
    gate = torch.rand(S, generator=torch.Generator().manual_seed(3))
    ga, be = rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1)
    rows_d, res_d, gate_d, ln_d = dev(rows), dev(res), dev(gate), (dev(ga), dev(be), 1e-5)
    rows64, res64, gate64, ga64, be64 = rows.double(), res.double(), gate.double().view(S, 1), ga.double(), be.double()
    out_null = torch.empty(S, D, device="cuda")
    worst_plain, worst_ln, calls = 0.0, 0.0, 0
    lib = _lib.load()
    for kind in ("identity", "permutation", "dropped", "all_dropped"):
        mp = _mapping(kind, S, seed=D + S)
        mp_d = dev(mp)
        m = mp.long()
        picked = torch.where((m >= 0).view(S, 1), rows64[m.clamp(min=0)], torch.zeros(S, D, dtype=torch.float64))
        for alpha in (1.0, 0.5):
            for use_g in (False, True):
                term = alpha * (gate64 if use_g else 1.0) * picked              # the fp64 reference is shared by the inner combinations
                for use_r in (False, True):
                    y64 = term + res64 if use_r else term
                    bound_plain = 4 * U * (term.abs() + res64.abs() if use_r else term.abs())
                    for use_ln in (False, True):
                        kw = dict(gate_value=gate_d if use_g else None, resid=res_d if use_r else None, alpha=alpha, ln=ln_d if use_ln else None)
                        go, gb = G.flat_out((S, D)), G.flat_out((S, D), torch.bfloat16)
                        ops.moe_combine(rows_d, mp_d, out=go.view, out_bf16=gb.view, **kw)
                        out_plain = ops.moe_combine(rows_d, mp_d, **kw)
                        g_, b_, eps = kw["ln"] if use_ln else (None, None, 0.0)
                        rc = lib.m3_moe_combine_bf16(_ptr(rows_d), _ptr(mp_d), _ptr(kw["gate_value"]), _ptr(kw["resid"]), float(alpha), _ptr(g_),
                                                     _ptr(b_), float(eps), _ptr(out_null), None, S, D, _stream())
                        assert rc == 0
                        torch.cuda.synchronize()
                        calls += 1
                        tag = "combine D=%d S=%d %s alpha=%g gate=%d resid=%d ln=%d" % (D, S, kind, alpha, use_g, use_r, use_ln)
                        go.check(tag + " out")
                        gb.check(tag + " out_bf16")
                        assert not bool(go.untouched().any()) and not bool(gb.untouched().any()), tag
                        assert G.same_bits(go.view, out_plain) and G.same_bits(go.view, out_null), tag + ": the three entry forms differ"
                        assert G.same_bits(gb.view, go.view.to(torch.bfloat16)), tag + ": out_bf16 is not out rounded to bf16"
                        got = go.view.cpu().double()
                        if use_ln:
                            want = F.layer_norm(y64, (D,), ga64, be64, 1e-5)
                            err = (got - want).abs()
                            worst_ln = max(worst_ln, float(err.max()))
                            assert bool((err <= 1e-5 + 1e-5 * want.abs()).all()), tag + ": max err %.3e" % float(err.max())
                        else:
                            err = (got - y64).abs()
                            nz = bound_plain > 0
                            if bool(nz.any()):
                                worst_plain = max(worst_plain, 4 * float((err[nz] / bound_plain[nz]).max()))
                            assert bool((err <= bound_plain).all()), tag + ": max err %.3e" % float(err.max())
    print("combine D=%d S=%d: %d calls, worst %.2f u of (|term| + |resid|) without LayerNorm (bound 4), worst abs err %.3e with (bound 1e-5)"
          % (D, S, calls, worst_plain, worst_ln))


@pytest.mark.parametrize("entry", ["m3_moe_combine", "m3_moe_combine_bf16"])
@pytest.mark.parametrize("D", [2052, 6])
def test_moe_combine_rejects_bad_width(D, entry):
    """launch_moe_combine: D a multiple of 4 and <= 2048, checked on the host before the launch (the buffers are large enough
    for either width all the same)"""
    S = 4
    rows, mp = torch.zeros(S, 2052, device="cuda"), torch.arange(S, dtype=torch.int32, device="cuda")
    out, ob = torch.zeros(S, 2052, device="cuda"), torch.zeros(S, 2052, dtype=torch.bfloat16, device="cuda")
    lib = _lib.load()
    with pytest.raises(M3Error):
        if entry == "m3_moe_combine":
            _lib.check(lib.m3_moe_combine(_ptr(rows), _ptr(mp), None, None, 1.0, None, None, 0.0, _ptr(out), S, D, _stream()), entry)
        else:
            _lib.check(lib.m3_moe_combine_bf16(_ptr(rows), _ptr(mp), None, None, 1.0, None, None, 0.0, _ptr(out), _ptr(ob), S, D, _stream()), entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,E,mode", [(50, 32, "uniform"), (200, 32, "with_dropped"), (2048, 32, "uniform"), (1500, 8, "with_dropped")])
def test_fused_expert_epilogue_equals_combine(S, E, mode):
    """ops.moe_expert_ffn(..., gate_value, resid, alpha, ln) == ops.moe_combine on the un-fused ops.moe_expert_ffn output
    scattered by mapping, bit for bit: short batches (slab kernel, F/64 slices summed by the combine) and long ones (>= 1024
    rows: the two grouped tiled GEMMs).  The un-fused call sums b2 and the slices in the same order and multiplies by
    alpha * gate = 1 exactly, so the second combine sees the very rows the fused one formed in registers."""
    D, Fh = 512, 1024
    rng = np.random.default_rng(S + E)
    g = torch.from_numpy((rng.integers(0, E, S) if mode == "uniform" else rng.integers(-1, E, S)).astype(np.int32))
    x = rnd(S, D, seed=1)
    w1, b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
    w2, b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
    gate, res = torch.rand(S, generator=torch.Generator().manual_seed(6)), rnd(S, D, seed=7)
    ga, be = rnd(D, seed=8) * 0.2 + 1.0, rnd(D, seed=9, scale=0.1)
    args = [dev(t) for t in (x, g, w1, b1, w2, b2)]
    kw = dict(gate_value=dev(gate), resid=dev(res), alpha=0.5, ln=(dev(ga), dev(be), 1e-12))
    fused = ops.moe_expert_ffn(*args, **kw)
    y = ops.moe_expert_ffn(*args)
    mapping, acc, _ = ops.moe_scatter_mapping(args[1], E)
    rows = ops.moe_local_scatter(y, mapping, S)
    two_step = ops.moe_combine(rows, mapping, **kw)
    assert G.same_bits(fused, two_step), "max diff %.3e" % float((fused - two_step).abs().max())
    assert bool((y.cpu()[g < 0] == 0).all())


# ================================================================================================ m3_layer_norm
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 4099])
@pytest.mark.parametrize("D", [4, 252, 256, 260, 512, 1024, 2048])
def test_layer_norm_sweep(D, rows):
    """m3_layer_norm over its four instantiations (D <= 256 / 512 / 1024 / 2048) and the 4-rows-per-work-group tail, eps 1e-12
    and 1e-5, inputs at (mean, std) = (0, 1), (1.5, 3), (100, 1); fp64 reference; x and y flat-guarded.
    layernorm_kernel is TWO-pass (mean first, then the sum of (x - mean)^2 on the registers), so the variance does not cancel
    and the error is flat in |mean| / std apart from one term: the mean itself is an fp32 sum of D values of size |mean|, off
    by a few u |mean|, which moves every output by that / std (and x - mean is exact only up to the rounding of mean).
    Bound: 1e-5 / 1e-5 (test_linear_layernorm_prologue) at (0, 1) and (1.5, 3).  The offset case (100, 1) is new and that bound
    is too tight for ANY fp32 evaluation of it: torch's fp32 LayerNorm on the CPU is off by 0.8e-5 (D = 4) .. 2.7e-5 (D = 260,
    4099 rows) against fp64 there.  So at (100, 1) the bound is 1e-5 + 1e-5 |ref| + 2 x that CPU fp32-vs-fp64 error, taken at the
    same shape and data (factor 2: another summation order); both figures are printed.  D = 4 rows have 4 samples: rows whose own std is below
    0.1 are excluded there (the 1 / std factor of LayerNorm amplifies input rounding without bound)."""
    worst = {}
    for eps in (1e-12, 1e-5):
        for mean, std in ((0.0, 1.0), (1.5, 3.0), (100.0, 1.0)):
            x = rnd(rows, D, seed=D + rows) * std + mean
            ga, be = rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1)
            gx, gy = G.flat_in(x), G.flat_out((rows, D))
            ga_d, be_d = dev(ga), dev(be)                     # (kept alive: the raw call below only takes their addresses)
            rc = _lib.load().m3_layer_norm(_ptr(gx.view), _ptr(ga_d), _ptr(be_d), float(eps), _ptr(gy.view), rows, D, _stream())
            assert rc == 0
            y_d = ops.layer_norm(dev(x), ga_d, be_d, eps)
            torch.cuda.synchronize()
            gy.check("layer_norm D=%d rows=%d" % (D, rows))
            assert not bool(gy.untouched().any())
            assert G.same_bits(gy.view, y_d)
            want = F.layer_norm(x.double(), (D,), ga.double(), be.double(), eps)
            err = (gy.view.cpu().double() - want).abs()
            bound = 1e-5 + 1e-5 * want.abs()
            if mean == 100.0:
                e32 = float((F.layer_norm(x, (D,), ga, be, eps).double() - want).abs().max())
                bound = bound + 2 * e32
                worst["eps=%g (%g,%g) CPU fp32" % (eps, mean, std)] = e32
            ok = err <= bound
            if D == 4:
                ok |= (x.double().std(1, unbiased=False) < 0.1 * std).view(rows, 1)
            worst["eps=%g (%g,%g)" % (eps, mean, std)] = float(err.max())
            assert bool(ok.all()), "layer_norm D=%d rows=%d eps=%g mean=%g std=%g: max err %.3e" % (D, rows, eps, mean, std, float(err.max()))
    print("layer_norm D=%d rows=%d max err: %s" % (D, rows, ", ".join("%s: %.2e" % kv for kv in worst.items())))


# ================================================================================================ expert-parallel index kernels
def _routing(law, S, world, e_loc, rng):
    E = world * e_loc
    if law == "uniform":
        return rng.integers(0, E, S)
    if law == "one_peer":                          # everything to the last rank (capacity = S is exactly enough)
        return (world - 1) * e_loc + rng.integers(0, e_loc, S)
    return rng.integers(-1, E, S)                  # with dropped rows


@pytest.mark.parametrize("S", [1, 50, 1090, 4400])
@pytest.mark.parametrize("world,e_loc", [(1, 32), (2, 16), (4, 8), (8, 8), (8, 4)])
def test_ep_send_map_and_recv_gate(world, e_loc, S):
    """m3_ep_send_map / m3_ep_recv_gate against ep_send_map_ref / ep_recv_gate_ref, bit-exact on map_send, on the e_loc
    counts of every header row and on gate_recv; everything else in the wire (pre-filled with the guard pattern: payload
    rows and the rest of the header rows) untouched by send_map.  capacity = S; row_bytes 2048 and the smallest legal
    max(16, 4 e_loc rounded up to 16).  Then the round trip: local_scatter(x, map_send) into the wire, ep_recv_gate on it,
    and every occupied wire row holds a token whose gate_idx % e_loc is the row's local expert id.
    Integer guards: gate_idx 0x7fffffff (outside [0, world e_loc): such a row is dropped), mapping / acc_histogram
    0x7fffffff (only enter arithmetic whose result is compared with capacity); none of them can become an address."""
    rng = np.random.default_rng(1000 * world + 10 * e_loc + S)
    E, cap = world * e_loc, S
    BIG = 0x7FFFFFFF
    for law in ("uniform", "one_peer", "dropped"):
        g = _routing(law, S, world, e_loc, rng).astype(np.int32)
        m_ref, a_ref = moe_index_ref(g, E)
        for row_bytes in (2048, max(16, -(-4 * e_loc // 16) * 16)):
            W = row_bytes // 4
            want_map, want_hdr = ep_send_map_ref(g, m_ref, a_ref, world, e_loc, cap, W)
            gg = G.flat_in(torch.from_numpy(g), int_guard=BIG)
            gm = G.flat_in(torch.from_numpy(m_ref), int_guard=BIG)
            ga = G.flat_in(torch.from_numpy(a_ref), int_guard=BIG)
            g_map = G.flat_out((S,), torch.int32)
            wire = G.flat_out((world, 1 + cap, W), torch.int32)
            ops.ep_send_map(gg.view, gm.view, ga.view, world, e_loc, cap, g_map.view, wire.view)
            torch.cuda.synchronize()
            tag = "ep world=%d e_loc=%d S=%d %s row_bytes=%d" % (world, e_loc, S, law, row_bytes)
            g_map.check(tag + " map_send")
            wire.check(tag + " wire")
            assert np.array_equal(g_map.view.cpu().numpy(), want_map), tag
            w_host = wire.view.cpu().numpy()
            assert np.array_equal(w_host[:, 0, :e_loc], want_hdr[:, 0, :e_loc]), tag
            untouched = wire.untouched().cpu().numpy()
            assert untouched[:, 1:, :].all() and untouched[:, 0, e_loc:].all(), tag + ": send_map wrote outside the header counts"
            # receive side on the same wire (world = 1 semantics per chunk: chunk j came from rank j)
            g_recv = G.flat_out((world * (1 + cap),), torch.int32)
            hdr_only = np.zeros_like(want_hdr)
            hdr_only[:, 0, :e_loc] = w_host[:, 0, :e_loc]
            ops.ep_recv_gate(wire.view, world, e_loc, cap, g_recv.view)
            torch.cuda.synchronize()
            g_recv.check(tag + " gate_recv")
            want_recv = ep_recv_gate_ref(hdr_only, world, e_loc, cap)
            assert np.array_equal(g_recv.view.cpu().numpy(), want_recv), tag
            # round trip: token ids ride in the payload
            x = torch.arange(S, dtype=torch.int32).view(S, 1).repeat(1, W).contiguous().cuda()
            flat_wire = wire.view.view(world * (1 + cap), W)
            ops.moe_local_scatter_into(x, g_map.view, flat_wire)
            torch.cuda.synchronize()
            wire.check(tag + " wire after scatter")
            recv = g_recv.view.cpu().numpy()
            tok = flat_wire[:, 0].cpu().numpy()
            occ = recv >= 0
            assert int(occ.sum()) == int((g >= 0).sum()), tag
            assert np.array_equal(recv[occ], g[tok[occ]] % e_loc), tag
            assert np.array_equal(np.sort(tok[occ]), np.nonzero(g >= 0)[0]), tag


# ================================================================================================ dense-ABI operators, guarded
@pytest.mark.parametrize("B,T,D,K", [(1, 7, 64, 15), (1, 9, 64, 15), (73, 7, 64, 15), (3, 171, 512, 15), (1, 5, 64, 7), (2, 3, 32, 15)])
def test_dwconv_ln_silu_guarded(B, T, D, K):
    """m3_dwconv_ln_silu at B * T one below / above a multiple of 8 rows (7, 9, 511, 513: 8 frames per work-group from 512
    rows on) and at T < K; bound of test_dwconv_ln_silu."""
    z, w, b = rnd(B, T, D, seed=1), rnd(D, 1, K, seed=2, scale=0.3), rnd(D, seed=3, scale=0.1)
    g, be = rnd(D, seed=4) * 0.2 + 1.0, rnd(D, seed=5, scale=0.1)
    gz, go = G.flat_in(z.view(B * T, D)), G.flat_out((B * T, D))
    wk, b_d, g_d, be_d = dev(w.squeeze(1).t().contiguous()), dev(b), dev(g), dev(be)
    rc = _lib.load().m3_dwconv_ln_silu(_ptr(gz.view), _ptr(wk), _ptr(b_d), _ptr(g_d), _ptr(be_d), 1e-5, B, T, D, K, _ptr(go.view), _stream())
    assert rc == 0
    out_d = ops.dwconv_ln_silu(dev(z.view(B * T, D)), wk, b_d, g_d, be_d, 1e-5, B, T)
    torch.cuda.synchronize()
    go.check("dwconv out")
    assert not bool(go.untouched().any()) and G.same_bits(go.view, out_d)
    y = F.conv1d(z.double().transpose(1, 2), w.double(), b.double(), padding=(K - 1) // 2, groups=D).transpose(1, 2)
    y = F.layer_norm(y, (D,), g.double(), be.double(), 1e-5)
    err = (go.view.cpu().double() - (y * torch.sigmoid(y)).reshape(B * T, D)).abs()
    print("dwconv B=%d T=%d: max err %.3e" % (B, T, float(err.max())))
    assert bool((err <= 2e-5 + 2e-5 * y.abs().reshape(B * T, D)).all())


@pytest.mark.parametrize("S,D", [(1, 4), (50, 512), (1023, 512), (1025, 36)])
def test_local_scatter_gather_guarded(S, D):
    """m3_moe_local_scatter / _gather: the mapping guard is an in-range row (0) -- a consumed guard would copy a wrong row, not
    address outside the buffers."""
    rng = np.random.default_rng(S + D)
    g = rng.integers(-1, 32, S).astype(np.int32)
    m_ref, a_ref = moe_index_ref(g, 32)
    n = max(int(a_ref[32]), 1)
    x = rng.standard_normal((S, D)).astype(np.float32)
    gx, gm = G.flat_in(torch.from_numpy(x)), G.flat_in(torch.from_numpy(m_ref), int_guard=0)
    gb = G.flat_out((n, D))
    ops.moe_local_scatter_into(gx.view, gm.view, gb.view)
    torch.cuda.synchronize()
    gb.check("local_scatter out")
    hit = np.zeros(n, dtype=bool)
    hit[m_ref[m_ref >= 0]] = True
    got = gb.view.cpu().numpy()
    assert np.array_equal(got[hit], local_scatter_ref(x, m_ref, n)[hit])
    assert bool(gb.untouched().cpu().numpy()[~hit].all())            # rows no token maps to keep their content
    buf = torch.from_numpy(local_scatter_ref(x, m_ref, n))
    gbuf, gout = G.flat_in(buf), G.flat_out((S, D))
    rc = _lib.load().m3_moe_local_gather(_ptr(gbuf.view), _ptr(gm.view), S, D * 4, _ptr(gout.view), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    gout.check("local_gather out")
    assert np.array_equal(gout.view.cpu().numpy(), local_gather_ref(buf.numpy(), m_ref))


@pytest.mark.parametrize("S", [1, 1023, 1024, 1025])
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_expert_ffn_guarded(S, wdt):
    """m3_moe_expert_ffn / _bf16 around the switch from the slab kernel to the grouped tiled GEMMs (1024 rows), x / gate_idx /
    y flat-guarded and the workspace guarded at exactly m3_moe_expert_workspace_size bytes.  gate_idx guard: expert 0 (in
    range; a consumed guard row would be computed with a wrong expert, never address past the weights).  References and
    bounds of test_fmoe_expert (3e-5 / 3e-5) and test_fmoe_expert_bf16 (fp64 on the bf16-rounded operands with H rounded to
    bf16: 1e-3 relative + 1e-3 of the output scale)."""
    E, D, Fh = 8, 512, 1024
    rng = np.random.default_rng(S)
    g = torch.from_numpy(rng.integers(-1, E, S).astype(np.int32))
    if S == 1:
        g[0] = 3
    x = rnd(S, D, seed=1)
    w1, b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
    w2, b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
    need = ops.moe_expert_workspace_size(S, E, D, Fh)
    gx, gg, gy, ws = G.flat_in(x), G.flat_in(g, int_guard=0), G.flat_out((S, D)), G.flat_out((need,), torch.uint8)
    wargs = [dev(t) for t in (w1.to(wdt), b1, w2.to(wdt), b2)]
    ops.moe_expert_ffn(gx.view, gg.view, *wargs, out=gy.view, workspace=ws.view)
    y_d = ops.moe_expert_ffn(dev(x), dev(g), *wargs)
    torch.cuda.synchronize()
    gy.check("expert_ffn y")
    ws.check("expert_ffn workspace")
    assert not bool(gy.untouched().any()) and G.same_bits(gy.view, y_d)
    if wdt == torch.float32:
        y_ref, _, _ = ref.fmoe_expert(x.view(1, S, D), g.view(1, S, 1), w1, b1, w2, b2)
        y_ref = y_ref.view(S, D).double()
        rtol, atol = 3e-5, 3e-5
    else:
        r16 = lambda t: t.float().to(torch.bfloat16).double()
        y_ref = torch.zeros(S, D, dtype=torch.float64)
        for e in range(E):
            sel = (g == e).nonzero().flatten()
            if sel.numel():
                h = F.silu(r16(x[sel]) @ r16(w1[e]).t() + b1[e].double())
                y_ref[sel] = r16(h) @ r16(w2[e]).t() + b2[e].double()
        rtol, atol = 1e-3, 1e-3 * float(y_ref.abs().max())
    err = (gy.view.cpu().double() - y_ref).abs()
    print("expert_ffn S=%d %s: max err %.3e" % (S, wdt, float(err.max())))
    assert bool((err <= atol + rtol * y_ref.abs()).all())
    assert bool((gy.view.cpu()[g < 0] == 0).all())


def _q8(t):
    """round-to-nearest-even to e4m3, saturating (test_fp8_gpu._q8)"""
    return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double()


@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 4096, 4097])
@pytest.mark.parametrize("form", ["w8", "w8a8"])
def test_expert_ffn_fp8_guarded(S, form):
    """m3_moe_expert_ffn_fp8 (e4m3 weights, bf16 arithmetic) and m3_moe_expert_ffn_fp8a8 (h_scale given) with x / gate_idx / y
    flat-guarded and the workspace guarded at exactly m3_moe_expert_workspace_size bytes: around 1024 rows (slab kernel ->
    grouped tiled GEMMs; fp8a8 runs the weight-only form below 4096 rows, so both forms share reference and bound there:
    test_fmoe_expert_fp8, 1e-3 of the output scale) and at 4096 / 4097 rows with 8 experts, where fp8a8 is the fused fp8
    kernel (m3_moe_expert_ffn_fp8a8_active) with the reference and row-error quantiles of test_fmoe_expert_fp8_arithmetic."""
    from m3asr.plan import quantize_fp8_rows
    E, D, Fh = 8, 512, 1024
    rng = np.random.default_rng(S)
    g = torch.from_numpy(rng.integers(-1, E, S).astype(np.int32))
    if S == 1:
        g[0] = 3
    x = rnd(S, D, seed=1)
    w1, b1 = rnd(E, Fh, D, seed=2, scale=D ** -0.5), rnd(E, Fh, seed=3, scale=0.1)
    w2, b2 = rnd(E, D, Fh, seed=4, scale=Fh ** -0.5), rnd(E, D, seed=5, scale=0.1)
    q1, s1 = quantize_fp8_rows(w1, dims=(2,))
    q2, s2 = quantize_fp8_rows(w2, dims=(2,))
    sel = [(g == e).nonzero().flatten() for e in range(E)]
    kw = dict(w1_scale=dev(s1), w2_scale=dev(s2))
    fused = False
    if form == "w8a8":
        hmax = max([float(F.silu(x[r] @ w1[e].t() + b1[e]).abs().max()) for e, r in enumerate(sel) if r.numel()])
        kw["h_scale"] = hmax * 1.25 / 448.0
        fused = _lib.load().m3_moe_expert_ffn_fp8a8_active(S, E, D, Fh) == 1
        assert fused == (S >= 4096)
    need = ops.moe_expert_workspace_size(S, E, D, Fh)
    gx, gg, gy, ws = G.flat_in(x), G.flat_in(g, int_guard=0), G.flat_out((S, D)), G.flat_out((need,), torch.uint8)
    wargs = [dev(t) for t in (q1, b1, q2, b2)]
    ops.moe_expert_ffn(gx.view, gg.view, *wargs, out=gy.view, workspace=ws.view, **kw)
    y_d = ops.moe_expert_ffn(dev(x), dev(g), *wargs, **kw)
    torch.cuda.synchronize()
    gy.check("expert_ffn fp8 y")
    ws.check("expert_ffn fp8 workspace")
    assert not bool(gy.untouched().any()) and G.same_bits(gy.view, y_d)
    r16 = lambda t: t.float().to(torch.bfloat16).double()
    want = torch.zeros(S, D, dtype=torch.float64)
    for e, r in enumerate(sel):
        if not r.numel():
            continue
        if fused:
            amax = x[r].abs().amax(1, keepdim=True).clamp_min(1e-30)
            xq, sx = _q8(x[r] * (448.0 / amax)), (amax * (1.0 / 448.0)).double()
            z = (xq @ q1[e].double().t()) * (s1[e].double() * sx) + b1[e].double()
            hq = _q8(F.silu(z).float() * (1.0 / kw["h_scale"]))
            want[r] = (hq @ q2[e].double().t()) * (s2[e].double() * kw["h_scale"]) + b2[e].double()
        else:
            h = F.silu((r16(x[r]) @ q1[e].double().t()) * s1[e].double() + b1[e].double())
            want[r] = (r16(h) @ q2[e].double().t()) * s2[e].double() + b2[e].double()
    scale = float(want.abs().max())
    row_err = ((gy.view.cpu().double() - want).abs().amax(1) / scale).numpy()
    live = (g >= 0).numpy()
    print("expert_ffn %s S=%d (fused fp8 kernel: %s): max row error %.3e of the output scale" % (form, S, fused, float(row_err.max())))
    if fused:
        q50, q90, qmax = (float(np.quantile(row_err[live], q)) for q in (0.5, 0.9, 1.0))
        assert q50 < 2e-4 and q90 < 4e-3 and qmax < 4e-2, (q50, q90, qmax)
    else:
        assert float(row_err.max()) < 1e-3, float(row_err.max())
    assert bool((gy.view.cpu()[g < 0] == 0).all())


@pytest.mark.parametrize("B,T,idim,C", [(1, 207, 40, 512), (2, 41, 40, 32), (2, 61, 40, 64), (3, 7, 40, 32)])
def test_subsampling_convs_guarded(B, T, idim, C):
    """m3_subsample_conv1 / m3_subsample_conv2 at odd T (the last input frame is not used by the stride-2 window; 7 frames give one
    output frame), inputs NaN-guarded, outputs pattern-guarded, bit-identical to the dense calls; bounds of test_subsampling_convs."""
    lib = _lib.load()
    feat = torch.rand(B, T, idim, generator=torch.Generator().manual_seed(1))
    w0, b0 = rnd(C, 1, 3, 3, seed=2, scale=1 / 3), rnd(C, seed=3, scale=0.1)
    w2, b2 = rnd(C, C, 3, 3, seed=4, scale=(9 * C) ** -0.5), rnd(C, seed=5, scale=0.1)
    T1, F1 = (T - 3) // 2 + 1, (idim - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    w0_d, b0_d, w2_d, b2_d = dev(w0.reshape(C, 9).t().contiguous()), dev(b0), dev(w2.permute(0, 2, 3, 1).contiguous()), dev(b2)
    gf, g1 = G.flat_in(feat), G.flat_out((B, T1, F1, C))
    assert lib.m3_subsample_conv1(_ptr(gf.view), _ptr(w0_d), _ptr(b0_d), B, T, idim, C, _ptr(g1.view), _stream()) == 0
    c1_d = ops.subsample_conv1(dev(feat), w0_d, b0_d)
    torch.cuda.synchronize()
    g1.check("subsample_conv1 out")
    assert not bool(g1.untouched().any()) and G.same_bits(g1.view, c1_d)
    y1 = F.relu(F.conv2d(feat.double().unsqueeze(1), w0.double(), b0.double(), stride=2))
    e1 = (g1.view.cpu().double() - y1.permute(0, 2, 3, 1)).abs()
    assert bool((e1 <= 1e-5 + 1e-5 * y1.permute(0, 2, 3, 1).abs()).all()), float(e1.max())
    gi, g2 = G.flat_in(c1_d.cpu()), G.flat_out((B, T2, F2, C))
    assert lib.m3_subsample_conv2(_ptr(gi.view), _ptr(w2_d), _ptr(b2_d), B, T1, F1, C, _ptr(g2.view), _stream()) == 0
    c2_d = ops.subsample_conv2(c1_d, w2_d, b2_d)
    torch.cuda.synchronize()
    g2.check("subsample_conv2 out")
    assert not bool(g2.untouched().any()) and G.same_bits(g2.view, c2_d)
    y2 = F.relu(F.conv2d(c1_d.cpu().double().permute(0, 3, 1, 2), w2.double(), b2.double(), stride=2)).permute(0, 2, 3, 1)
    e2 = (g2.view.cpu().double() - y2).abs()
    print("subsampling B=%d T=%d C=%d: conv1 max err %.3e, conv2 max err %.3e" % (B, T, C, float(e1.max()), float(e2.max())))
    assert bool((e2 <= 3e-5 + 3e-5 * y2.abs()).all()), float(e2.max())


def test_small_row_ops_guarded():
    """m3_cmvn, m3_log_softmax_bias, m3_ctc_topk on flat-guarded inputs and outputs (row counts that do not fill the last
    work-group), each bit-identical to the dense call."""
    lib = _lib.load()
    B, T, D = 3, 13, 80
    x, lens = rnd(B, T, D, seed=1), torch.tensor([13, 7, 1], dtype=torch.int32)
    mean, istd = rnd(D, seed=2), torch.rand(D, generator=torch.Generator().manual_seed(3)) + 0.5
    gx, gy = G.flat_in(x), G.flat_out((B, T, D))
    lens_d, mean_d, istd_d = dev(lens), dev(mean), dev(istd)
    assert lib.m3_cmvn(_ptr(gx.view), _ptr(lens_d), _ptr(mean_d), _ptr(istd_d), B, T, D, _ptr(gy.view), _stream()) == 0
    y_d = ops.cmvn(dev(x), lens_d, mean_d, istd_d)
    torch.cuda.synchronize()
    gy.check("cmvn")
    live = (torch.arange(T).view(1, T) < lens.view(B, 1))
    assert G.same_bits(gy.view[live.cuda()], y_d[live.cuda()])
    want = (x.double() - mean.double()) * istd.double()
    assert bool(((gy.view.cpu().double() - want).abs()[live] <= 1e-6 + 1e-6 * want.abs()[live]).all())

    rows, V = 37, 1434
    lg, bias = rnd(rows, V, seed=4, scale=3.0), rnd(V, seed=5)
    gl, go = G.flat_in(lg), G.flat_out((rows, V))
    bias_d = dev(bias)
    assert lib.m3_log_softmax_bias(_ptr(gl.view), _ptr(bias_d), _ptr(go.view), rows, V, _stream()) == 0
    o_d = ops.log_softmax_bias(dev(lg), bias_d)
    torch.cuda.synchronize()
    go.check("log_softmax_bias")
    assert not bool(go.untouched().any()) and G.same_bits(go.view, o_d)
    want = torch.log_softmax(lg.double(), -1) + bias.double()
    assert bool(((go.view.cpu().double() - want).abs() <= 1e-5 + 1e-5 * want.abs()).all())

    k = 10
    gp, gi = G.flat_out((rows, k)), G.flat_out((rows, k), torch.int32)
    assert lib.m3_ctc_topk(_ptr(gl.view), rows, V, k, _ptr(gp.view), _ptr(gi.view), _stream()) == 0
    p_d, i_d = ops.ctc_topk(dev(lg), k)
    torch.cuda.synchronize()
    gp.check("ctc_topk logp")
    gi.check("ctc_topk idx")
    assert torch.equal(gi.view, i_d) and G.same_bits(gp.view, p_d)
    wp, wi = torch.log_softmax(lg.double(), -1).topk(k, -1)
    assert torch.equal(gi.view.cpu().long(), wi)
    assert bool(((gp.view.cpu().double() - wp).abs() <= 1e-5 + 1e-5 * wp.abs()).all())
