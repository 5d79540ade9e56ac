"""The attention decoder's device kernels called one by one (csrc/aed_rescore.hip, csrc/aed_search.hip) against the float64
mirrors of tests/aed_kernels_ref.py: every head size of both attention kernels, the 64-key / 16-query / 4-query tile edges, the
self-attention cache across its 64-position tile, the skip and frozen rules bit for bit, ties and non-finite logits, and every
leading dimension with live garbage behind the row end (tests/guarded.py).

Yardstick, that of tests/test_aed_rescore_gpu.py but PER OUTPUT ELEMENT: the mirror in float64 is the truth, e32 is the largest
error of the same mirror in float32 on the CPU on the test's own inputs, the device must be within max(8 e32, 1e-5).  No bound
comes from the device's output; every test prints device error, e32 and bound before it asserts (run with -s).  Tokens, parents,
flags, best, steps and targets must be identical; tests/test_aed_kernels_host.py asserts for every synthetic case that each
decision is decided by more than twice the bound or is an exact tie by construction.  Bytes that must not change are compared
bit for bit."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import aed_kernels_ref as kref
import aed_search_ref as sref
import guarded
from m3asr import _lib, ops

DKS = [16, 32, 48, 64, 80, 96, 112, 128]
dk_id = lambda d: "dk%d" % d   # noqa: E731


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


def _within(tag, dev, r64, r32):
    """print device error, e32 and bound of one output, then assert the yardstick element by element"""
    e32, bound = kref.yardstick(r64, r32)
    err = kref.max_err(dev.cpu(), r64)
    print("%s: device err %.3e, e32 %.3e, bound %.3e" % (tag, err, e32, bound))
    assert err <= bound, (tag, err, bound)
    return bound


def _rows_written(tag, g, wrote):
    """the rows of a guarded (rows, width) output the kernel must write hold no pattern, the others nothing but the pattern"""
    g.check(tag)
    u = g.untouched().cpu()
    assert not bool(u[wrote].any()), tag + ": a row the kernel must write still holds the fill pattern"
    assert bool(u[~wrote].all()), tag + ": a row the kernel must skip was written"


# ------------------------------------------------------------------------------------------------------ m3_aed_attention
@pytest.mark.parametrize("dk", DKS, ids=dk_id)
def test_attention_head_sizes_and_tile_edges(dk):
    """one launch, H = 2: the slots of kref.ATT_SLOTS (keys 63 / 64 / 65 / 129, queries 15 / 16 / 17 / 33, causal 16 / 17 / 65),
    a shared key range, five skip slots, two twins; q / k / v with three leading dimensions, ldo > D, NaN in every unused row"""
    H = 2
    c = kref.attention_case(H, dk)
    D = H * dk
    gq, gk = guarded.strided_in(c["q"], ld=D + 8), guarded.strided_in(c["k"], ld=D + 12)
    gv, go = guarded.strided_in(c["v"], ld=D + 20), guarded.strided_out(c["q_rows"], D, ld=D + 9)
    assert len({gq.ld, gk.ld, gv.ld}) == 3 and go.ld > D
    ops.aed_attention(gq.view, gk.view, gv.view, _i32(c["desc"]), c["max_q"], H, out=go.view)
    torch.cuda.synchronize()
    r64, wrote = kref.attention(c["q"].double(), c["k"].double(), c["v"].double(), c["desc"], H)
    r32, _ = kref.attention(c["q"], c["k"], c["v"], c["desc"], H)
    _rows_written("aed_attention dk %d" % dk, go, wrote)
    for slot, (r0, n) in c["skipped"].items():
        assert not bool(wrote[r0:r0 + n].any())
    out = guarded.dense(go.view).cpu()
    _within("aed_attention dk %d, %d slots" % (dk, len(c["live"])), out[wrote], r64[wrote], r32[wrote])
    for a, b in c["twins"]:
        (qa, n), qb = c["desc"][a][:2], c["desc"][b][0]
        assert guarded.same_bits(out[qa:qa + n], out[qb:qb + n]), "slot %d and its copy at slot %d differ" % (a, b)


def test_attention_fused_qkv_h8():
    """H = 8, dk = 64 on the driver's layout: q | k | v are column blocks of one buffer, ldq = ldk = ldv = 3 D"""
    c = kref.fused_attention_case()
    H, D = c["H"], c["H"] * c["dk"]
    g = guarded.strided_in(c["qkv"], ld=3 * D + 8)
    go = guarded.strided_out(c["rows"], D, ld=D + 9)
    q, k, v = g.view[:, :D], g.view[:, D:2 * D], g.view[:, 2 * D:]
    ops.aed_attention(q, k, v, _i32(c["desc"]), c["max_q"], H, out=go.view)
    torch.cuda.synchronize()
    parts = [c["qkv"][:, i * D:(i + 1) * D] for i in range(3)]
    r64, wrote = kref.attention(*[p.double() for p in parts], c["desc"], H)
    r32, _ = kref.attention(*parts, c["desc"], H)
    _rows_written("aed_attention fused", go, wrote)
    out = guarded.dense(go.view).cpu()
    _within("aed_attention fused qkv, H 8, dk 64", out[wrote], r64[wrote], r32[wrote])


# ----------------------------------------------------------------------------------------------- m3_aed_search_attention
def _state(case, D, H, layers=1):
    desc = ops.aed_search_desc(case["B"], case["beam"], case["max_steps"], case["V"], D, H, layers, case["pe_rows"])
    state = torch.zeros(ops.aed_search_state_size(desc) // 4, dtype=torch.int32, device="cuda")
    return desc, state


def _logits(case):
    steps, R, V = case["logits"].shape
    return guarded.strided_in(case["logits"].reshape(steps * R, V), ld=V + 9)      # NaN behind every row's end


@pytest.mark.parametrize("mem_len", [(1, 63, 64, 65), (130, 1, 2, 64)], ids=lambda m: "mem" + "_".join(map(str, m)))
@pytest.mark.parametrize("dk", DKS, ids=dk_id)
def test_search_attention_source(dk, mem_len):
    """B = 4, beam = 3, memories at non-monotone non-zero rows.  Launch A: everybody live.  Then one prune: the utterance with
    one frame is done (limit 1).  Launch B with one key row less than utterance 3 needs: the done utterance's rows and the
    rows of the utterance whose range runs past kv_rows are bit-untouched, the other two are compared."""
    B, N, H, V = 4, 3, 2, 7
    D, R = H * dk, B * N
    g = torch.Generator().manual_seed(dk + sum(mem_len))
    row0, at = [0] * B, 5
    for u in (2, 0, 1, 3):
        row0[u] = at
        at += mem_len[u] + 3
    kv_rows = row0[3] + mem_len[3]
    kv = torch.randn(kv_rows, 2 * D, generator=g)
    logits = kref.grid_logits(g, R, V)
    for r in range(R):
        kref.place_eos(logits[r], None)
    case = dict(B=B, beam=N, V=V, max_steps=4, pe_rows=8, logits=logits.view(1, R, V))
    desc, state = _state(case, D, H)
    ops.aed_search_reset(desc, state, _i32(row0), _i32(mem_len))
    gkv = guarded.strided_in(kv, ld=2 * D + 12)
    done_u = mem_len.index(1)
    for launch, (rows_given, live) in enumerate([(kv_rows, [0, 1, 2, 3]), (kv_rows - 1, [u for u in (0, 1, 2) if u != done_u])]):
        q = torch.randn(R, D, generator=g)
        gq, go = guarded.strided_in(q, ld=D + 8), guarded.strided_out(R, D, ld=D + 9)
        ops.aed_search_attention(desc, state, gq.view, gkv.view[:rows_given], go.view, 0)
        torch.cuda.synchronize()
        wrote = torch.tensor([r // N in live for r in range(R)])
        _rows_written("aed_search_attention source", go, wrote)
        r64 = kref.search_source_attention(q.double(), kv.double(), row0, mem_len, N, H)
        r32 = kref.search_source_attention(q, kv, row0, mem_len, N, H)
        _within("aed_search_attention source dk %d mem %s launch %d" % (dk, mem_len, launch), guarded.dense(go.view).cpu()[wrote],
                r64[wrote], r32[wrote])
        if launch == 0:
            done = _i32([0] * B)
            ops.aed_search_prune(desc, state, _logits(case).view, done)
            assert done.tolist() == [int(u == done_u) for u in range(B)]


def _run_self(dk, case, layers, check_steps, H=2):
    """Self use over the whole of a synthetic search: per step and layer one launch on fresh random q and K | V rows, then the
    step's prune.  Every launch: the cache changed in the slice (layer, step, live rows) alone, which holds the rows' K | V bit for
    bit (the other layer, later positions, the rows of done utterances and the guards keep what they held); the rows of done
    utterances keep the output pattern.  At the steps of check_steps `out` is compared with the mirror."""
    B, N, steps = case["B"], case["beam"], case["logits"].shape[0]
    D, R = H * dk, B * N
    desc, state = _state(case, D, H, layers)
    ops.aed_search_reset(desc, state, _i32([7 * u for u in range(B)]), _i32(case["mem_len"]))
    trace = kref.run_search(case, torch.float64)
    g = torch.Generator().manual_seed(dk + steps)
    q_all, kv_all = torch.randn(steps, layers, R, D, generator=g), torch.randn(steps, layers, R, 2 * D, generator=g)
    gq, gkv = guarded.strided_in(q_all.view(-1, D), ld=D + 8), guarded.strided_in(kv_all.view(-1, 2 * D), ld=2 * D + 12)
    glog = _logits(case)
    cache = guarded.flat_out((layers, case["max_steps"], R, 2 * D))
    assert cache.view.numel() * 4 == ops.aed_search_cache_size(desc)
    done = _i32([0] * B)
    worst = 0.0
    for s in range(steps):
        live = [u for u in range(B) if not trace[s][u]["done"]]
        wrote = torch.tensor([r // N in live for r in range(R)])
        for layer in range(layers):
            i = (s * layers + layer) * R
            go = guarded.strided_out(R, D, ld=D + 9)
            expect = cache.buf.clone()
            if live:
                ev = expect[cache.origin:cache.origin + cache.view.numel()].view(cache.view.shape)
                ev[layer, s, wrote.cuda()] = kv_all[s, layer][wrote].cuda()
            ops.aed_search_attention(desc, state, gq.view[i:i + R], gkv.view[i:i + R], go.view, layer, cache=cache.view)
            torch.cuda.synchronize()
            assert guarded.same_bits(cache.buf, expect), "step %d layer %d: the cache differs outside the step's slice or in it" % (s, layer)
            _rows_written("aed_search_attention self step %d" % s, go, wrote)
            if s in check_steps and live:
                hist = [trace[s][u]["history"] for u in range(B)]
                r64 = kref.search_self_attention(q_all[s, layer].double(), [kv_all[t, layer].double() for t in range(s + 1)], hist, s, N, H, live)
                r32 = kref.search_self_attention(q_all[s, layer], [kv_all[t, layer] for t in range(s + 1)], hist, s, N, H, live)
                bound = _within("aed_search_attention self dk %d B %d step %d layer %d" % (dk, B, s, layer),
                                guarded.dense(go.view).cpu()[wrote], r64[wrote], r32[wrote])
                worst = max(worst, bound)
        ops.aed_search_prune(desc, state, glog.view[s * R:(s + 1) * R], done)
    # the device took the mirror's picks: same tokens, so the same ancestry was under test
    res = ops.aed_search_result(desc, state)
    for u in range(B):
        want = sref.result(trace[-1][u], case["V"] - 1)
        assert res["steps"][u].item() == want["steps"]
        for j, (toks, _, _) in enumerate(want["nbest"]):
            assert res["hyp_tokens"][u, j, :len(toks)].tolist() == list(toks) and res["hyp_len"][u, j].item() == len(toks)
    return worst


@pytest.mark.parametrize("dk", DKS, ids=dk_id)
def test_search_attention_self_short(dk):
    """B = 2, beam = 3, 2 layers, 5 steps whose picks permute and duplicate parents (asserted on the host)"""
    _run_self(dk, kref.walk_case(2, 5), layers=2, check_steps=range(5))


@pytest.mark.parametrize("B", [1, 2], ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("dk", [16, 80, 128], ids=dk_id)
def test_search_attention_self_across_the_tile(dk, B):
    """70 steps, nobody finishes: n_keys = s + 1 passes 64 at s = 63; positions 63, 64 and 65 are live"""
    _run_self(dk, kref.walk_case(B, 70), layers=1, check_steps=(0, 1, 62, 63, 64, 65, 69))


def test_search_attention_done_utterance_stores_nothing():
    """utterance 0 (3 frames) is done after step 2 next to a live one: at steps 3 and 4 none of its rows is stored or written"""
    _run_self(16, kref.walk_case(2, 5, mem_len=(3, 9)), layers=2, check_steps=range(5))


# ------------------------------------------------------------------------- m3_aed_search_reset / _embed / _prune / _result
def _compare_result(tag, res, states, case, r32_states):
    """m3_aed_search_result against the states of one step: the discrete outputs identical, the scores by the yardstick"""
    N, eos, S = case["beam"], case["V"] - 1, case["max_steps"]
    res = {k: v.cpu() for k, v in res.items()}
    for u, st in enumerate(states):
        want = sref.result(st, eos)
        for j, (toks, _, fin) in enumerate(want["nbest"]):
            assert res["hyp_tokens"][u, j].tolist() == list(toks) + [-1] * (S - len(toks)), (tag, u, j)
            assert res["hyp_len"][u, j].item() == len(toks) and res["finished"][u, j].item() == int(fin), (tag, u, j)
        assert res["best"][u].item() == want["best"] and res["steps"][u].item() == want["steps"], (tag, u)
    s64, s32 = torch.stack([st["score"] for st in states]), torch.stack([st["score"] for st in r32_states])
    return res["score"], s64, s32


def _run_steps(case, D, H):
    B, N, V = case["B"], case["beam"], case["V"]
    R, steps = B * N, case["logits"].shape[0]
    P = case["max_steps"] + 1
    rec = 2 + 2 * P                                                  # csrc/aed_search_state.h: score, finished, tokens[P], path[P]
    desc, state = _state(case, D, H)
    ops.aed_search_reset(desc, state, _i32([11 * u + 3 for u in range(B)]), _i32(case["mem_len"]), max_steps=case["reset_steps"])
    t64, t32 = kref.run_search(case, torch.float64), kref.run_search(case, torch.float32)
    g = torch.Generator().manual_seed(V + D)
    emb, pe = torch.randn(V, D, generator=g), torch.randn(case["pe_rows"], D, generator=g)
    emb_d, pe_d = emb.cuda(), pe.cuda()
    glog = _logits(case)
    dev_scores, x_dev, x64, x32 = [], [], [], []
    sc = _compare_result("reset", ops.aed_search_result(desc, state), t64[0], case, t32[0])
    dev_scores.append(sc[0])
    for s in range(steps):
        live = [u for u in range(B) if not t64[s][u]["done"]]
        wrote = torch.tensor([r // N in live for r in range(R)])
        gx = guarded.strided_out(R, D, ld=D + 9)
        ops.aed_search_embed(desc, state, emb_d, pe_d, gx.view)
        before = state.clone()
        gdone = guarded.flat_out((B,), torch.int32)
        ops.aed_search_prune(desc, state, glog.view[s * R:(s + 1) * R], gdone.view)
        torch.cuda.synchronize()
        _rows_written("aed_search_embed step %d" % s, gx, wrote)
        if live:
            last = torch.tensor([(t64[s][r // N]["tokens"][r % N] or [V - 1])[-1] for r in range(R)])
            pos = torch.tensor([t64[s][r // N]["steps"] for r in range(R)])
            x_dev.append(guarded.dense(gx.view).cpu()[wrote])
            x64.append((emb.double()[last] * math.sqrt(D) + pe.double()[pos])[wrote])
            x32.append((emb[last] * math.sqrt(D) + pe[pos])[wrote])
        gdone.check("done")
        assert gdone.view.tolist() == [int(st["done"]) for st in t64[s + 1]], "done words after launch %d" % s
        # frozen: the header and both records of every row of an utterance that was done before the launch, bit for bit
        for u in range(B):
            if t64[s][u]["done"]:
                assert torch.equal(before[8 * u:8 * u + 8], state[8 * u:8 * u + 8]) and before[8 * u + 2].item() == 1
                lo = 8 * B + u * N * 2 * rec
                assert torch.equal(before[lo:lo + N * 2 * rec], state[lo:lo + N * 2 * rec]), "launch %d changed done utterance %d" % (s, u)
        sc = _compare_result("launch %d" % s, ops.aed_search_result(desc, state), t64[s + 1], case, t32[s + 1])
        dev_scores.append(sc[0])
    _within("%s scores, %d launches" % (case["name"], steps), torch.stack(dev_scores), kref.search_scores(t64), kref.search_scores(t32))
    _within("%s embed rows, D %d" % (case["name"], D), torch.cat(x_dev), torch.cat(x64), torch.cat(x32))


@pytest.mark.parametrize("beam,V", kref.SEARCH_SHAPES, ids=lambda x: str(x))
def test_search_steps(beam, V):
    """reset / embed / prune / result on synthetic logits, B = 3 with limits 1, 4 and 7 (reset with fewer steps than the
    descriptor), ldl > V, ldx > D; after every launch tokens, scores, flags, best, steps and done, and the frozen utterances"""
    _run_steps(kref.search_case(beam, V), 32, 2)


def test_search_steps_wide_embed():
    """the same at D = 2048: the embed rows have more columns than a work-group has threads"""
    _run_steps(kref.search_case(3, 11), 2048, 16)


def test_search_ties():
    """equal logits in a row -> the lower token id; equal scores under identical rows -> the lower flat index; equal final
    scores -> the first slot is best (kref.tie_case; what must come out is asserted on the host)"""
    _run_steps(kref.tie_case(), 32, 2)


def test_search_nonfinite_logits():
    """-inf logits, a NaN in a row, fewer than beam non-NaN logits, a row of NaN, the -inf slots of step 0: the pick order as
    include/m3asr.h words it (kref.nonfinite_step)"""
    _run_steps(kref.nonfinite_case(), 32, 2)


# ----------------------------------------------------------------------------------------------------------- m3_aed_embed
def _embed_inputs(V, pe_rows, F):
    """B = 3, beam = 4.  utterance 0: hypotheses of 0, 1 and 9 tokens, slot 3 past n_hyps with a stale length.  utterance 1:
    n_hyps = -1, stale lengths.  utterance 2: a token outside [0, V); a slot whose row range disagrees with its length; a slot
    that needs more than pe_rows positions; an ordinary one.  Dead and disagreeing slots get row ranges that fit their stale
    lengths, so that only the rule under test keeps the kernel off them."""
    g = torch.Generator().manual_seed(4)
    lens = [[0, 1, 9, 5], [2, 2, 2, 2], [2, 3, pe_rows, 3]]
    given = [[1, 2, 10, 6], [3, 3, 3, 3], [3, 5, pe_rows + 1, 4]]      # rows allotted: len + 1, but 5 for the length 3 of (2, 1)
    tokens = torch.full((3, 4, F), -1, dtype=torch.int32)
    for b in range(3):
        for i in range(4):
            tokens[b, i, :lens[b][i]] = torch.randint(0, V - 1, (lens[b][i],), generator=g).to(torch.int32)
    tokens[2, 0, 1] = V + 3
    row0 = [0]
    for b in range(3):
        for i in range(4):
            row0.append(row0[-1] + given[b][i])
    return tokens, torch.tensor(lens, dtype=torch.int32), torch.tensor([3, -1, 4], dtype=torch.int32), torch.tensor(row0, dtype=torch.int32)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("D", [4, 32, 2048], ids=lambda d: "D%d" % d)
def test_embed(D, reverse):
    V, pe_rows, F, B, beam = 11, 10, 12, 3, 4
    tokens, lens, n_hyps, row0 = _embed_inputs(V, pe_rows, F)
    rows = int(row0[-1])
    g = torch.Generator().manual_seed(D)
    emb, pe = torch.randn(V, D, generator=g), torch.randn(pe_rows, D, generator=g)
    gx, gt = guarded.strided_out(rows, D, ld=D + 9), guarded.flat_out((rows,), torch.int32)
    dev = [t.cuda() for t in (tokens, lens, n_hyps, row0, emb, pe)]
    _lib.check(_lib.load().m3_aed_embed(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), B, beam, F, _ptr(dev[4]), _ptr(dev[5]),
                                        pe_rows, V, D, int(reverse), rows, _ptr(gx.view), gx.ld, _ptr(gt.view), _stream()), "m3_aed_embed")
    torch.cuda.synchronize()
    x64, target, wrote = kref.embed(tokens, lens, n_hyps, row0, emb.double(), pe.double(), rows, reverse)
    x32, _, _ = kref.embed(tokens, lens, n_hyps, row0, emb, pe, rows, reverse)
    assert wrote.tolist() == [True] * 13 + [False] * 18 + [True] * 3 + [False] * 16 + [True] * 4
    _rows_written("aed_embed x", gx, wrote)
    gt.check("target")
    assert bool(gt.untouched().cpu()[~wrote].all()) and gt.view.cpu()[wrote].tolist() == target[wrote].tolist()
    assert (V + 3) in target[wrote].tolist() and int(torch.isnan(x64).any(1).sum()) == 1
    _within("aed_embed D %d %s" % (D, "reverse" if reverse else "forward"), guarded.dense(gx.view).cpu()[wrote], x64[wrote], x32[wrote])


# ----------------------------------------------------------------------------------------------------------- m3_aed_score
def _final_margin(final, best):
    """smallest gap between an utterance's best final score and another one that is not bit-identical to it"""
    m = kref.INF
    for b, arg in enumerate(best):
        for j, f in enumerate(final[b].tolist()):
            if arg >= 0 and j != arg and f == f and f != float(final[b, arg]):
                m = min(m, abs(float(final[b, arg]) - f))
    return m


@pytest.mark.parametrize("bi", [False, True], ids=["left", "bi_prior"])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1434], ids=lambda v: "V%d" % v)
def test_score_logits(V, bi):
    """one-row hypotheses (B = 2, beam = 4, 7 rows): att IS the row's log-probability, checked element by element, and so is the
    row_logp scratch, in guarded buffers with ldl > V and ldrl > V; one target outside [0, V) gives NaN"""
    B, beam, rows = 2, 4, 7
    g = torch.Generator().manual_seed(V + int(bi))
    logits, r_logits = torch.randn(rows, V, generator=g) * 3, torch.randn(rows, V, generator=g) * 3
    target, r_target = torch.randint(0, V, (rows,), generator=g), torch.randint(0, V, (rows,), generator=g)
    target[2] = V + 2
    r_target[5] = -1
    prior = -torch.rand(B, beam, generator=g) * 10
    row0, n_hyps = list(range(8)) + [7], [4, 3]
    cw, rw = (0.5, 0.3) if bi else (0.0, 0.0)
    gl, grl = guarded.strided_in(logits, ld=V + 9), guarded.strided_in(r_logits, ld=V + 13)
    gt, grt = guarded.flat_in(target.to(torch.int32), int_guard=-7), guarded.flat_in(r_target.to(torch.int32), int_guard=-7)
    glp = guarded.flat_out((2 * rows,))
    gatt, gratt, gfin = (guarded.flat_out((B, beam)) for _ in range(3))
    gbest = guarded.flat_out((B,), torch.int32)
    row0_d, n_hyps_d, prior_d = _i32(row0), _i32(n_hyps), prior.cuda()          # named: they must outlive the call
    _lib.check(_lib.load().m3_aed_score(_ptr(gl.view), gl.ld, _ptr(grl.view) if bi else None, grl.ld, _ptr(gt.view),
                                        _ptr(grt.view) if bi else None, _ptr(row0_d), _ptr(n_hyps_d), _ptr(prior_d), B, beam,
                                        rows, V, cw, rw, _ptr(glp.view), _ptr(gatt.view), _ptr(gratt.view), _ptr(gfin.view),
                                        _ptr(gbest.view), _stream()), "m3_aed_score")
    torch.cuda.synchronize()
    want = [kref.score(logits.to(dt), r_logits.to(dt) if bi else None, target, r_target, row0, n_hyps, prior, B, beam, cw, rw)
            for dt in (torch.float64, torch.float32)]
    for gbuf in (glp, gatt, gratt, gfin, gbest):
        gbuf.check("aed_score")
    n_lp = 2 * rows if bi else rows
    assert bool(glp.untouched()[n_lp:].all()) and not bool(glp.untouched()[:n_lp].any())
    tag = "aed_score V %d %s" % (V, "bi + prior" if bi else "left")
    bound = 0.0
    for name, gbuf, i in (("row_logp", glp, 0), ("att", gatt, 1), ("r_att", gratt, 2), ("final", gfin, 3)):
        dev = gbuf.view.cpu()[:n_lp] if i == 0 else gbuf.view.cpu()
        bound = max(bound, _within(tag + " " + name, dev, want[0][i], want[1][i]))
    assert int(torch.isnan(want[0][1]).sum()) == 1 and float(want[0][1][1, 3]) == -kref.INF
    margin = _final_margin(want[0][3], want[0][4])
    print("%s: best margin %.3e (2 x bound %.3e)" % (tag, margin, 2 * bound))
    assert margin > 2 * bound and gbest.view.tolist() == want[0][4]


@pytest.mark.parametrize("beam", [1, 4, 64], ids=lambda b: "beam%d" % b)
def test_score_hypotheses(beam):
    """B = 4 through ops.aed_score: multi-row hypotheses (sums in row order), dead slots (-inf in all three outputs), n_hyps = 0
    and -1 (best = -1), and an utterance whose first two finals tie bit for bit at the top (best = the first)"""
    B, V = 4, 65
    g = torch.Generator().manual_seed(beam)
    counts = [min(beam, 3), 0, -1, beam]
    lens = [[2, 0, 5][:counts[0]], [], [], [1] * beam]
    row0 = [0]
    for b in range(B):
        for i in range(beam):
            row0.append(row0[-1] + (lens[b][i] + 1 if i < len(lens[b]) else 0))
    rows = row0[-1]
    logits, r_logits = torch.randn(rows, V, generator=g) * 2, torch.randn(rows, V, generator=g) * 2
    target, r_target = torch.randint(0, V, (rows,), generator=g), torch.randint(0, V, (rows,), generator=g)
    prior = -torch.rand(B, beam, generator=g)
    if beam > 1:                                                      # utterance 3: slots 0 and 1 identical and far ahead
        a, b2 = row0[3 * beam], row0[3 * beam + 1]
        for t in (logits, r_logits):
            t[a:a + 2, :] = torch.randn(2, V, generator=g)
            t[a, int(target[a])] = t[a + 1, int(target[a + 1])] = 12.0
        r_target[a:a + 2] = target[a:a + 2]
        for t in (logits, r_logits, target, r_target):
            t[b2:b2 + 2] = t[a:a + 2]
        prior[3, 1] = prior[3, 0]
    gl, grl = guarded.strided_in(logits, ld=V + 9), guarded.strided_in(r_logits, ld=V + 13)
    for bi, cw, rw in ((False, 0.0, 0.0), (True, 0.5, 0.3)):
        att, r_att, final, best = ops.aed_score(gl.view, _i32(target), _i32(row0), _i32(counts), B, beam, prior=prior.cuda(), ctc_weight=cw,
                                                r_logits=grl.view if bi else None, r_target=_i32(r_target) if bi else None, reverse_weight=rw)
        torch.cuda.synchronize()
        want = [kref.score(logits.to(dt), r_logits.to(dt) if bi else None, target, r_target, row0, counts, prior, B, beam, cw, rw)
                for dt in (torch.float64, torch.float32)]
        tag = "aed_score beam %d %s" % (beam, "bi + prior" if bi else "left")
        bound = max(_within(tag + " " + name, dev, want[0][i], want[1][i]) for name, dev, i in (("att", att, 1), ("r_att", r_att, 2), ("final", final, 3)))
        margin = _final_margin(want[0][3], want[0][4])
        print("%s: best margin %.3e (2 x bound %.3e)" % (tag, margin, 2 * bound))
        assert want[0][4][1:3] == [-1, -1] and want[0][4][3] == 0 and bool((want[0][1][1:3] == -kref.INF).all())
        assert beam == 1 or float(want[0][3][3, 0]) == float(want[0][3][3, 1])
        assert margin > 2 * bound and best.tolist() == want[0][4]


def test_score_without_rows():
    """rows = 0: nobody has a hypothesis; every output is still written"""
    B, beam, V = 2, 4, 9
    att, r_att, final, best = ops.aed_score(torch.zeros(0, V, device="cuda"), _i32([]), _i32([0] * (B * beam + 1)), _i32([0, -1]), B, beam)
    torch.cuda.synchronize()
    for t in (att, r_att, final):
        assert bool((t.cpu() == -kref.INF).all())
    assert best.tolist() == [-1, -1]
