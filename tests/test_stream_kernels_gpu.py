"""The two stateful kernels of chunk-by-chunk decoding, and the dense causal conv, called alone (m3_relpos_attention_stream,
m3_dwconv_ln_silu_stream, m3_dwconv_ln_silu_causal; include/m3asr.h).

The engine tests reach these kernels only at chunk = 8 / 12 / 16 (one query tile), the default ring size, dk = 64 / 128, K = 15
with LayerNorm, and only through logits.  Here the test IS the stream: it writes `step` and `chunk_len` before every launch,
slices chunk n out of a full-sequence qkv and keeps p whole.  Each case is held to
  (a) an fp64 reference of the whole utterance (tests/stream_kernels_ref.py; its own fp32 error is measured on the CPU in
      test_stream_kernels_host.py), at the bound of the dense test of the same operator;
  (b) the full-utterance kernel under the same static chunk mask / the dense causal conv, bit for bit;
  (c) state: the K / V ring and the conv ping-pong pair hold exactly the frames they should, a NaN-initialised state never
      reaches an output, guards around strided / flat outputs keep their pattern (tests/guarded.py).
Cases and inputs: stream_kernels_ref.ATT_CASES / CONV_CASES.  Every test prints its worst error.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G
import stream_kernels_ref as R
from m3asr import ops, _lib

NAN = float("nan")


def dev(t):
    return None if t is None else t.cuda().contiguous()


def close(got, want, rtol, atol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    print("%s max abs err %.3e (max |ref| %.3e, bound %.1e / %.1e)" % (what, float(err.max()), float(want.abs().max()), rtol, atol))
    assert bool((err <= bound).all()), "%s max abs err %.3e (max |ref| %.3e), worst excess %.3e" % (
        what, float(err.max()), float(want.abs().max()), float((err - bound).max()))


# ================================================================================================ attention, lockstep
def _att_lockstep(d, strided):
    """All chunks of a case through m3_relpos_attention_stream with ONE counter.  strided: qkv is a guarded view with
    ldq = 3 D + 4, p a guarded view with the case's ldp (NaN rows follow its last row directly), out a guarded view with
    ldo = D + 4, fresh per launch and checked after it.  Returns (rows [B][Ttot][D], hist [B][cap][2 D]) on the device."""
    B, C, D = d.B, d.C, d.D
    hist = torch.full((B, d.cap, 2 * D), NAN, device="cuda")
    step, cl = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    u, v = dev(d.u), dev(d.v)
    if strided:
        pv = G.strided_in(d.p, ld=d.ldp).view
        gq = G.strided_in(torch.zeros(B * C, 3 * D), ld=3 * D + 4)
    else:
        pv = dev(d.p)
    rows = []
    for n in range(d.nchunks):
        chunk = d.qkv[:, n * C:(n + 1) * C].reshape(B * C, 3 * D)
        step.fill_(n)
        cl.copy_(d.chunk_lens[n])
        if strided:
            gq.view.copy_(chunk)
            go = G.strided_out(B * C, D, ld=D + 4)
            ops.relpos_attention_stream(gq.view, hist, pv, u, v, cl, step, B, C, d.H, d.dk, d.left, out=go.view)
            go.check("stream attention out, chunk %d" % n)
            assert not bool(go.untouched().any())
            rows.append(G.dense(go.view).view(B, C, D))
        else:
            rows.append(ops.relpos_attention_stream(dev(chunk), hist, pv, u, v, cl, step, B, C, d.H, d.dk, d.left).view(B, C, D))
    torch.cuda.synchronize()
    return torch.cat(rows, 1), hist


_lock_cache = {}


def _att_lockstep_dense(case):
    """(inputs, rows, hist) of a case on dense operands, computed once and shared (never modified)"""
    if case not in _lock_cache:
        d = R.att_inputs(case)
        _lock_cache[case] = (d,) + _att_lockstep(d, strided=False)
    return _lock_cache[case]


@pytest.mark.parametrize("case", R.ATT_CASES, ids=str)
def test_relpos_attention_stream_lockstep(case):
    """(a) fp64, 3e-5 / 3e-5 as test_relpos_attention; from 130 keys on the larger of that and 4 x the error of the formula in
    fp32 on the CPU, as test_relpos_attention_strided (printed).  (b) torch.equal with m3_relpos_attention_chunk(chunk = C) on
    the whole utterances, which is itself held to the fp64 reference (it has never run at these chunk sizes).  (c) hist starts
    as NaN: every output row, valid or not, is finite.  (d) after the last chunk, ring slot f % cap of every utterance holds
    K | V of frame f for the last min(cap, Ttot) frames APPENDED -- in lockstep every chunk appends its C rows of every
    utterance, finished or not (the rows at and past chunk_len are the finite values of the contract), so these are the frames
    of the padded sequence.  (e) guards hold, and the strided and the dense stream give the same bits, history included."""
    d, rows_d, hist_d = _att_lockstep_dense(case)
    B, C, D, T = d.B, d.C, d.D, d.Ttot
    args = (d.qkv.view(B * T, 3 * D), d.p, d.u, d.v, d.lens, B, T, d.H, d.dk, C, d.left)
    want = R.attention_ref(*args).view(B, T, D)
    tol = 3e-5
    if T >= 130:
        e32 = float((R.attention_ref(*args, dtype=torch.float32).double().view(B, T, D) - want)[d.valid].abs().max())
        tol = max(tol, 4 * e32)
        print("Ttot=%d: fp32 CPU reference error %.3e -> bound %.3e" % (T, e32, tol))
    rows, hist = _att_lockstep(d, strided=True)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(rows_d).all()), "a stale or never-written history slot was read"   # (c)
    got = rows.cpu()
    close(got[d.valid], want[d.valid], tol, tol, "stream attention %s" % (case,))                                                      # (a)
    full = ops.relpos_attention(dev(d.qkv.view(B * T, 3 * D)), dev(d.p), dev(d.u), dev(d.v), dev(d.lens), B, T, d.H, d.dk,
                                chunk=C, left_chunks=d.left).view(B, T, D).cpu()
    close(full[d.valid], want[d.valid], tol, tol, "full-utterance attention, chunk mask %d / %d" % (C, d.left))
    assert torch.equal(got[d.valid], full[d.valid]), "stream rows differ from the full-utterance kernel's: %.3e" % float(
        (got[d.valid] - full[d.valid]).abs().max())                                                                                    # (b)
    assert G.same_bits(rows, rows_d) and G.same_bits(hist, hist_d), "strided and dense streams differ"                                 # (e)
    f = torch.arange(T - min(d.cap, T), T)
    assert G.same_bits(hist[:, (f % d.cap).cuda()].cpu(), d.qkv[:, f, D:].contiguous()), "history ring does not hold the last frames"   # (d)


# ================================================================================================ slot schedules
# What each of the three slots does per launch ("tick").  run: decode the slot's next chunk and advance its counter;
# restart: step = 0 and a fresh state first, then run; the others are the three causes of a slot not being live, with the
# slot's rows holding finite random values and its counter kept: len0 (chunk_len = 0: a pause), neg (chunk_len < 0),
# stepneg (step = -1), stepmax (step = slot_max_chunks).  Slot 1 starts two launches late, slot 2 pauses twice for one launch,
# slot 0 restarts mid-run: at tick 3 slot 2 is at chunk 2 and the others at chunks 3 and 1, so the counters differ in parity.
SCHEDULE = [["run"] * 4 + ["restart"] + ["run"] * 7,
            ["len0", "stepneg"] + ["run"] * 4 + ["stepmax"] + ["run"] * 5,
            ["run"] * 2 + ["len0", "run", "neg"] + ["run"] * 7]
NTICKS = 12


def _slot_tick(t, idx, chunk_lens, C, max_chunks):
    """-> per slot (kind, chunk index or None, chunk_len to write, step to write); idx is advanced for the slots that run"""
    plan = []
    for b in range(3):
        kind = SCHEDULE[b][t]
        if kind == "restart":
            idx[b] = 0
        if kind in ("run", "restart"):
            n = idx[b]
            if n < chunk_lens.shape[0] and int(chunk_lens[n, b]) > 0:
                plan.append((kind, n, int(chunk_lens[n, b]), n))
                idx[b] += 1
                continue
            kind = "len0"                                     # the utterance has ended: nothing to decode
        n = min(idx[b], max_chunks - 1)
        plan.append({"len0": (kind, None, 0, n), "neg": (kind, None, -3, n), "stepneg": (kind, None, C, -1),
                     "stepmax": (kind, None, C, max_chunks)}[kind])
    return plan


def test_relpos_attention_stream_slots():
    """Slot mode (one counter per slot) on the schedule above.  A live slot's valid rows are bit-equal to the lockstep
    stream's rows of the same utterance at the same chunk -- whatever the other slots do in that launch.  A slot that is not
    live, for each of the three causes, gets C rows of exact zeros and its history block keeps every bit.  The restarted
    slot's history is refilled with NaN first: nothing of its first life is read."""
    case = R.ATT_SLOT_CASE
    d, lock, _ = _att_lockstep_dense(case)
    B, C, D, maxc = d.B, d.C, d.D, d.nchunks
    assert B == 3 and maxc * C == d.p.shape[0]
    hist = torch.full((B, d.cap, 2 * D), NAN, device="cuda")
    step, cl = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    u, v = dev(d.u), dev(d.v)
    gp, gq = G.strided_in(d.p, ld=d.ldp), G.strided_in(torch.zeros(B * C, 3 * D), ld=3 * D + 4)
    idx, seen, lock_c = [0, 0, 0], set(), lock.cpu()
    for t in range(NTICKS):
        plan = _slot_tick(t, idx, d.chunk_lens, C, maxc)
        chunk = R.rnd(B, C, 3 * D, seed=100 + t)
        for b, (kind, n, nl, st) in enumerate(plan):
            if kind == "restart":
                hist[b].fill_(NAN)
            if n is not None:
                chunk[b] = d.qkv[b, n * C:(n + 1) * C]
        gq.view.copy_(chunk.view(B * C, 3 * D))
        cl.copy_(torch.tensor([p[2] for p in plan], dtype=torch.int32))
        step.copy_(torch.tensor([p[3] for p in plan], dtype=torch.int32))
        before = hist.clone()
        go = G.strided_out(B * C, D, ld=D + 4)
        ops.relpos_attention_stream(gq.view, hist, gp.view, u, v, cl, step, B, C, d.H, d.dk, d.left, slot_max_chunks=maxc, out=go.view)
        go.check("slot attention out, tick %d" % t)
        got = G.dense(go.view).view(B, C, D).cpu()
        for b, (kind, n, nl, st) in enumerate(plan):
            seen.add((b, kind))
            if n is not None:
                assert torch.equal(got[b, :nl], lock_c[b, n * C:n * C + nl]), "tick %d slot %d chunk %d differs from lockstep" % (t, b, n)
                assert bool(torch.isfinite(got[b]).all())
            else:
                assert bool((got[b] == 0).all()), "tick %d: slot %d (%s) is not live but got non-zero rows" % (t, b, kind)
                assert G.same_bits(hist[b], before[b]), "tick %d: slot %d (%s) is not live but its history changed" % (t, b, kind)
    assert {(0, "restart"), (1, "len0"), (1, "stepneg"), (1, "stepmax"), (2, "len0"), (2, "neg")} <= seen
    assert idx[0] == maxc                                     # the restarted slot decoded its whole utterance again
    print("slot attention: %d launches, live rows bit-equal to lockstep" % NTICKS)


# ================================================================================================ causal conv, stream form
def _conv_lockstep(d, check_cache=True):
    """All chunks through m3_dwconv_ln_silu_stream with ONE counter; half 0 of the pair starts as R, half 1 as NaN.  After
    every launch: the half the next chunk reads = the last K - 1 frames of [old cache | z[:chunk_len]] bit for bit, the half
    just read keeps every bit, the guard around the flat output holds.  Returns rows [nchunks][B][T][D] (CPU)."""
    B, T, D, K = d.B, d.T, d.D, d.K
    pair = torch.full((2, B, K - 1, D), NAN, device="cuda")
    pair[0] = d.R.cuda()
    cur = d.R.clone()
    step, cl = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    w = [dev(t) for t in (d.w_kc, d.bias, d.gamma, d.beta)]
    rows = []
    for n in range(d.z.shape[0]):
        step.fill_(n)
        cl.copy_(d.chunk_lens[n])
        go = G.flat_out((B * T, D))
        ops.dwconv_ln_silu_stream(dev(d.z[n].reshape(B * T, D)), *w, R.CONV_EPS, B, T, pair, step, cl, out=go.view)
        go.check("stream conv out, chunk %d" % n)
        assert not bool(go.untouched().any())
        rows.append(go.view.cpu().view(B, T, D))
        if check_cache:
            nxt = torch.stack([R.next_cache(cur[b], d.z[n, b], int(d.chunk_lens[n, b])) for b in range(B)])
            assert G.same_bits(pair[n & 1].cpu(), cur), "chunk %d: the cache half that was read changed" % n
            assert G.same_bits(pair[(n & 1) ^ 1].cpu(), nxt), "chunk %d: new cache is not the last K - 1 frames of [cache | z[:len]]" % n
            cur = nxt
    return torch.stack(rows)


def _conv_gather(rows, where):
    return torch.stack([rows[n, t] for n, t in where])


@pytest.mark.parametrize("case", R.CONV_CASES, ids=str)
def test_dwconv_ln_silu_stream_lockstep(case):
    """Random initial cache: every valid row against the fp64 causal conv + LayerNorm + SiLU over [R | z_0 | z_1 | ...] of
    its utterance, 2e-5 / 2e-5 as test_dwconv_ln_silu; the cache pair after every launch (see _conv_lockstep).
    Broadcast initial cache (every row = left_fill): the stream's valid rows are bit-equal to ONE m3_dwconv_ln_silu_causal
    call over the whole padded utterances, which is held to the same reference."""
    d = R.conv_inputs(case)
    rows = _conv_lockstep(d)
    assert bool(torch.isfinite(rows).all()), "the NaN half of the cache pair reached an output"
    for b, (want, where) in enumerate(R.conv_stream_ref(d)):
        close(_conv_gather(rows[:, b], where), want, 2e-5, 2e-5, "stream conv %s utterance %d" % (case, b))

    f = R.conv_inputs(case, broadcast_fill=True)
    rows_f = _conv_lockstep(f)
    B, T, D, nch = f.B, f.T, f.D, f.z.shape[0]
    zfull = R.rnd(B, nch * T, D, seed=9)                      # padded utterances: valid frames first, finite values behind them
    refs = R.conv_stream_ref(f)
    for b, (_, where) in enumerate(refs):
        zfull[b, :len(where)] = _conv_gather(f.z[:, b], where)
    go = G.flat_out((B * nch * T, D))
    ops.dwconv_ln_silu_causal(dev(zfull.view(-1, D)), dev(f.w_kc), dev(f.bias), dev(f.gamma), dev(f.beta), R.CONV_EPS, dev(f.fill), B, nch * T,
                              out=go.view)
    go.check("causal conv out")
    full = go.view.cpu().view(B, nch * T, D)
    for b, (want, where) in enumerate(refs):
        close(full[b, :len(where)], want, 2e-5, 2e-5, "causal conv %s utterance %d" % (case, b))
        assert torch.equal(_conv_gather(rows_f[:, b], where), full[b, :len(where)]), "stream and whole-utterance causal conv differ"


@pytest.mark.parametrize("B,T,D,K,ln", [(1, 5, 36, 15, True), (2, 36, 512, 15, True), (7, 99, 32, 7, False), (3, 200, 36, 31, True)])
def test_dwconv_ln_silu_causal(B, T, D, K, ln):
    """m3_dwconv_ln_silu_causal alone against fp64 (2e-5 / 2e-5): the (B, T) of test_dwconv_ln_silu's small shapes and one
    launch of 600 rows (>= 512 rows, the regime that test names); flat guarded output."""
    z, fill = R.rnd(B, T, D, seed=1), R.rnd(D, seed=7)
    w_kc, bias = R.rnd(K, D, seed=2, scale=0.3), R.rnd(D, seed=3, scale=0.1)
    gamma, beta = (R.rnd(D, seed=4) * 0.2 + 1.0, R.rnd(D, seed=5, scale=0.1)) if ln else (None, None)
    go = G.flat_out((B * T, D))
    gz = G.flat_in(z.view(B * T, D))
    ops.dwconv_ln_silu_causal(gz.view, dev(w_kc), dev(bias), dev(gamma), dev(beta), R.CONV_EPS, dev(fill), B, T, out=go.view)
    go.check("causal conv out")
    assert not bool(go.untouched().any())
    want = torch.stack([R.causal_conv_ref(torch.cat([fill.view(1, D).expand(K - 1, D), z[b]]), w_kc, bias, gamma, beta) for b in range(B)])
    close(go.view.cpu().view(B, T, D), want, 2e-5, 2e-5, "causal conv B=%d T=%d D=%d K=%d" % (B, T, D, K))


def test_dwconv_ln_silu_stream_slots():
    """Slot mode on the schedule of the attention test.  A slot that is not live (each cause) keeps every bit of BOTH halves
    of its pair.  A live slot reads the half its OWN counter's parity names (at tick 3 the slots' parities differ), its
    valid rows are bit-equal to the lockstep stream's at the same chunk, and the half it writes is the last K - 1 frames of
    [its cache | z[:chunk_len]].  A restarted slot gets R in half 0 and NaN in half 1 again."""
    case, nch = R.CONV_SLOT_CASE, 5
    d = R.conv_inputs(case, nchunks=nch)
    d = d._replace(B=3, z=d.z[:, :3].contiguous(), R=d.R[:3].contiguous(),
                   chunk_lens=torch.tensor([[16, 16, 16], [16, 16, 16], [16, 1, 16], [16, 0, 13], [16, 0, 0]], dtype=torch.int32))
    lock = _conv_lockstep(d)
    B, T, D, K, maxc = 3, d.T, d.D, d.K, 8
    pair = torch.full((2, B, K - 1, D), NAN, device="cuda")
    pair[0] = d.R.cuda()
    cur = [d.R[b].clone() for b in range(B)]
    step, cl = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    w = [dev(t) for t in (d.w_kc, d.bias, d.gamma, d.beta)]
    idx, seen = [0, 0, 0], set()
    for t in range(NTICKS):
        plan = _slot_tick(t, idx, d.chunk_lens, T, maxc)
        z = R.rnd(B, T, D, seed=100 + t)
        for b, (kind, n, nl, st) in enumerate(plan):
            if kind == "restart":
                pair[0, b], pair[1, b] = d.R[b].cuda(), NAN
                cur[b] = d.R[b].clone()
            if n is not None:
                z[b] = d.z[n, b]
        cl.copy_(torch.tensor([p[2] for p in plan], dtype=torch.int32))
        step.copy_(torch.tensor([p[3] for p in plan], dtype=torch.int32))
        before = pair.clone()
        go = G.flat_out((B * T, D))
        ops.dwconv_ln_silu_stream(dev(z.view(B * T, D)), *w, R.CONV_EPS, B, T, pair, step, cl, slot_max_chunks=maxc, out=go.view)
        go.check("slot conv out, tick %d" % t)
        got, after = go.view.cpu().view(B, T, D), pair.cpu()
        for b, (kind, n, nl, st) in enumerate(plan):
            seen.add((b, kind))
            if n is not None:
                assert torch.equal(got[b, :nl], lock[n, b, :nl]), "tick %d slot %d chunk %d differs from lockstep" % (t, b, n)
                nxt = R.next_cache(cur[b], d.z[n, b], nl)
                assert G.same_bits(after[n & 1, b], cur[b]) and G.same_bits(after[(n & 1) ^ 1, b], nxt), "tick %d slot %d: cache pair" % (t, b)
                cur[b] = nxt
            else:
                assert G.same_bits(after[:, b], before[:, b].cpu()), "tick %d: slot %d (%s) is not live but its cache pair changed" % (t, b, kind)
    assert {(0, "restart"), (1, "len0"), (1, "stepneg"), (1, "stepmax"), (2, "len0"), (2, "neg")} <= seen
    print("slot conv: %d launches, live rows bit-equal to lockstep" % NTICKS)


# ================================================================================================ rejections
def _P(t):
    return None if t is None else t.data_ptr()


def test_stream_entries_reject_bad_arguments():
    """Every refusal happens on the host (api.hip / the launchers' M3_REQUIRE) with a message and before any launch: the
    output and the state still hold their fill afterwards.  The same calls with legal arguments are accepted."""
    lib = _lib.load()
    B, C, H, dk, T, K = 2, 8, 2, 64, 8, 15
    D = H * dk
    z = lambda *s, **kw: torch.zeros(*s, device="cuda", **kw)
    qkv, p, u, hist = z(B * C, 3 * D + 4), z(64, D + 4), z(H, dk), z(B, 32, 2 * D)
    out, pair, zz, zo, wk = torch.full((B * C, D + 4), 7.0, device="cuda"), z(2, B, K - 1, D), z(B * T, D), z(B * T, D), z(K, D)
    one, per, cl = z(1, dtype=torch.int32), z(B, dtype=torch.int32), torch.full((B,), C, dtype=torch.int32, device="cuda")

    def att(**kw):
        a = dict(qkv=qkv, ldq=3 * D, hist=hist, cap=32, p=p, ldp=D, p_rows=64, u=u, v=u, cl=cl, step=one, B=B, C=C, H=H, dk=dk, left=1,
                 slots=-1, out=out, ldo=D, off=0)
        a.update(kw)
        return lib.m3_relpos_attention_stream(_P(a["qkv"]) + a["off"], a["ldq"], _P(a["hist"]), a["cap"], _P(a["p"]), a["ldp"], a["p_rows"],
                                              _P(a["u"]), _P(a["v"]), _P(a["cl"]), _P(a["step"]), a["B"], a["C"], a["H"], a["dk"],
                                              1.0 / math.sqrt(a["dk"]), a["left"], a["slots"], _P(a["out"]), a["ldo"], None)

    def conv(**kw):
        a = dict(z=zz, g=u.view(-1), pair=pair, step=one, cl=cl, D=D, K=K, slots=-1)
        a.update(kw)
        return lib.m3_dwconv_ln_silu_stream(_P(a["z"]), _P(wk), _P(u), _P(a["g"]), _P(a["g"]), 1e-5, B, T, a["D"], a["K"], _P(a["pair"]),
                                            _P(a["step"]), _P(a["cl"]), a["slots"], _P(zo), None)

    def causal(**kw):
        a = dict(fill=u.view(-1), D=D)
        a.update(kw)
        return lib.m3_dwconv_ln_silu_causal(_P(zz), _P(wk), _P(u), None, None, 1e-5, _P(a["fill"]), B, T, a["D"], K, _P(zo), None)

    assert att() == 0 and att(slots=8, step=per) == 0 and att(ldq=3 * D + 4, ldp=D + 4, ldo=D + 4) == 0
    assert conv() == 0 and conv(g=None) == 0 and conv(slots=8, step=per) == 0 and causal() == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    hist.fill_(3.0)
    pair.fill_(3.0)
    zo.fill_(5.0)
    bad_att = [dict(cap=4), dict(left=4, cap=32), dict(ldq=3 * D + 2), dict(ldp=D + 2), dict(dk=48), dict(hist=None), dict(step=None),
               dict(cl=None), dict(slots=9, step=per), dict(ldq=3 * D - 4), dict(ldp=D - 4), dict(ldo=D - 1), dict(off=4), dict(p_rows=4),
               dict(B=0), dict(out=None)]
    for kw in bad_att:
        assert att(**kw) != 0 and "attention (stream" in _lib.last_error(), kw
    for kw in [dict(slots=0, step=per), dict(D=30), dict(pair=None), dict(step=None), dict(cl=None), dict(K=1), dict(z=None)]:
        assert conv(**kw) != 0 and "dwconv" in _lib.last_error(), kw
    for kw in [dict(fill=None), dict(D=30)]:
        assert causal(**kw) != 0 and "dwconv" in _lib.last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((hist == 3.0).all()) and bool((pair == 3.0).all()) and bool((zo == 5.0).all()), "a rejected call launched"
