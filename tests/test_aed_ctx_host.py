"""CPU checks of tests/aed_ctx_ref.py, the restatement that attention decoding with hotword biasing on the device is held to
(tests/test_aed_ctx_gpu.py): against the restatements it extends, against ContextGraph.walk and a brute-force occurrence count,
on hand-built behaviours and against invariants of the search itself; the conditions the cases of tests/aed_ctx_cases.py were
picked for; what AttentionBeamSearch refuses before it touches a device; and the new exports."""
import ctypes
import os
import re
import types

import pytest
import torch

import aed_ctx_cases as cases
import aed_ctx_ref as ref
import aed_joint_cases
import aed_lm_cases
import aed_search_ref
from m3asr.context import ContextGraph, ContextSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SMALL = [n for n in cases.SPECS if n != "real"]


# ------------------------------------------------------------------------------- 1. unbiased: the restatements it extends
def _same_history(got, want, keys=("key", "att", "ctc")):
    for g, w in zip(got, want):
        assert g["best"] == w["best"] and g["margin"] == w["margin"] and g["steps"] == w["steps"] and g["limit"] == w["limit"]
        for eg, ew in zip(g["history"], w["history"]):
            for k in keys:
                assert torch.equal(eg[k], ew[k]), k
            assert eg["tokens"] == ew["tokens"] and eg["parent"] == ew["parent"] and eg["finished"] == ew["finished"]


@pytest.mark.parametrize("how", ["minus_one", "out_of_range", "empty_set"])
def test_unbiased_is_the_lm_search(how):
    """graph_ids = -1, an id past the set, or an empty set: aed_lm_ref's results on aed_lm_cases' tiny, exactly"""
    dcfg, sd, memory, mem_len, ctc, spec, lm, _ = aed_lm_cases.case("tiny")
    want = aed_lm_cases.reference("tiny")[0]
    g = ContextGraph([[8, 7], [5]], dcfg.vocab, score=2.0)
    graphs, ids = {"minus_one": ([g], [-1] * 3), "out_of_range": ([g], [1, 7, 1]), "empty_set": ([], None)}[how]
    got = ref.search(sd, dcfg, memory, mem_len, ctc, spec["beam"], spec["pre_beam"], spec["w"], lm, spec["alpha"], spec["beta"], graphs, ids,
                     spec["use_eos"], None, spec["max_steps"])
    _same_history(got, want)
    for gr, w in zip(got, want):
        assert [h[:6] for h in gr["nbest"]] == w["nbest"] and gr["lm_state"] == w["lm_state"] and gr["n"] == w["n"]
        assert all(h[6] == 0.0 and h[7] == 0.0 for h in gr["nbest"]) and gr["ctx_state"] == [0] * spec["beam"]
        for eg, ew in zip(gr["history"], w["history"]):
            assert eg["lm"] == ew["lm"] and eg["lm_state"] == ew["lm_state"]


def test_unbiased_without_lm_is_the_joint_search():
    dcfg, sd, memory, mem_len, ctc, spec = aed_joint_cases.case("tiny")
    want = aed_joint_cases.reference("tiny")[0]
    got = ref.search(sd, dcfg, memory, mem_len, ctc, spec["beam"], spec["pre_beam"], spec["w"], None, 0.0, 0.0, [], None, True, None,
                     spec["max_steps"])
    _same_history(got, want)
    for g, w in zip(got, want):
        assert [h[:5] for h in g["nbest"]] == w["nbest"]


def test_unbiased_without_lm_and_ctc_is_the_attention_search():
    """ctc_weight = 0, no LM, unbiased: the pre-beam does not change what the plain attention search keeps"""
    dcfg, sd, memory, mem_len, _, spec = aed_joint_cases.case("tiny")
    want = aed_search_ref.search(sd, dcfg, memory, mem_len, spec["beam"])
    g = ContextGraph([[8, 7]], dcfg.vocab, score=2.0)
    got = ref.search(sd, dcfg, memory, mem_len, None, spec["beam"], spec["pre_beam"], 0.0, None, 0.0, 0.0, [g], [-1, -1, -1])
    for gr, w in zip(got, want):
        assert [(h[0], h[1], h[4]) for h in gr["nbest"]] == w["nbest"] and gr["best"] == w["best"] and gr["steps"] == w["steps"]
        assert all(h[1] == h[2] and h[3] == 0.0 for h in gr["nbest"])
        for eg, ew in zip(gr["history"], w["history"]):
            assert torch.equal(eg["key"], ew["score"]) and eg["tokens"] == ew["tokens"] and eg["parent"] == ew["parent"]


# ------------------------------------------------------------------- 2. ContextGraph.walk and the brute-force occurrence count
def _occurrences(phrases, toks):
    return sum(len(p) for p in phrases for i in range(len(toks) - len(p) + 1) if tuple(toks[i:i + len(p)]) == tuple(p))


def _no_prefix(phrases):
    return not any(a != b and tuple(b[:len(a)]) == tuple(a) for a in phrases for b in phrases)


@pytest.mark.parametrize("name", SMALL)
def test_bonus_is_the_walk_and_the_occurrence_count(name):
    """every returned hypothesis: (ctx_state, bonus) == ContextGraph.walk over its tokens with eos stripped, bit for bit; a
    finished one holds walk's final in state 0; without a prefix phrase the final is the occurrence count times the score;
    and the carried state of every kept candidate of every step is the re-walked one"""
    dcfg, _, _, mem_len, _, spec, _, graphs = cases.case(name)
    eos = dcfg.vocab - 1
    gs = ref.graph_of(graphs, spec["ids"], len(mem_len))
    checked = 0
    for res, g in zip(cases.reference(name)[0], gs):
        for h, state, bonus, final in zip(res["nbest"], res["ctx_state"], res["bonus"], res["final"]):
            if g is None:
                assert (state, bonus, final) == (0, 0.0, 0.0)
                continue
            s, b, f = g.walk(h[0])
            if h[4]:
                assert (state, bonus, final) == (0, f, f), (h[0], bonus, f)
            else:
                assert (state, bonus, final) == (s, b, f), (h[0], bonus, b)
            assert h[6] == bonus and h[7] == final
            if _no_prefix(g.phrases):
                assert final == g.score * _occurrences(g.phrases, h[0])
            checked += 1
        for e in res["history"]:
            for toks, state, bonus, fin in zip(e["tokens"], e["ctx_state"], e["bonus"], e["finished"]):
                if g is None:
                    continue
                s, b, f = g.walk(aed_search_ref.strip(toks, eos))
                assert (state, bonus) == ((0, f) if fin else (s, b))
    assert checked >= spec["beam"]


# ------------------------------------------------------------------------------------------------- 3. hand-built behaviours
def _table(V, rows, tail_eos=0.9):
    """an attention model that needs no weights: the next-token probabilities depend on the hypothesis's length alone; rows[i] is
    a dict token -> probability for length i, the rest is spread evenly; past the table eos takes tail_eos"""
    def logp_of(tokens):
        given = rows[len(tokens)] if len(tokens) < len(rows) else {V - 1: tail_eos}
        rest = (1.0 - sum(given.values())) / (V - len(given))
        p = torch.full((V,), rest, dtype=torch.float64)
        for t, v in given.items():
            p[t] = v
        return torch.log(p)
    return logp_of


def _run(logp_of, V, limit, beam, P, graphs, ids=None):
    return ref.search_with([None], [logp_of], [limit], beam, P, 0.0, None, 0.0, 0.0, V - 1, graphs, ids)[0]


def test_the_best_hypothesis_flips_to_the_phrase():
    V = 6
    f = _table(V, [{1: 0.5, 2: 0.3}, {3: 0.5, 4: 0.3}, {V - 1: 0.9}])
    g = ContextGraph([[2, 4]], V, score=1.0)
    plain, biased = _run(f, V, 4, 3, 3, [g], [-1]), _run(f, V, 4, 3, 3, [g], [0])
    assert plain["nbest"][plain["best"]][0] == (1, 3) and biased["nbest"][biased["best"]][0] == (2, 4)
    top = biased["nbest"][biased["best"]]
    assert top[6] == 2.0 and top[7] == 2.0 and top[4]
    import math
    assert abs(top[2] - math.log(0.3 * 0.3 * 0.9)) < 1e-12 and abs(top[1] - (top[2] + 2.0)) < 1e-12
    assert plain["nbest"][plain["best"]][1] > top[2]                # without the graph the phrase's hypothesis loses


@pytest.mark.parametrize("end", ["token", "eos"])
def test_a_partial_match_is_retracted(end):
    """phrase (1, 2, 3): the path 1, 2, 4 loses its two credits at 4; the path 1, 2, eos loses them at eos"""
    V, w = 6, 1.5
    rows = [{1: 0.9}, {2: 0.9}, {4: 0.9} if end == "token" else {V - 1: 0.9}, {V - 1: 0.9}]
    g = ContextGraph([[1, 2, 3]], V, score=w)
    res = _run(_table(V, rows), V, 6, 1, 1, [g])
    bonus = [e["bonus"][0] for e in res["history"]]
    assert bonus[:3] == [w, 2 * w, 0.0] and res["nbest"][0][4] and res["nbest"][0][6] == 0.0 and res["ctx_state"] == [0]
    assert res["nbest"][0][0] == ((1, 2, 4) if end == "token" else (1, 2))
    keys = [float(e["key"][0]) for e in res["history"]]
    att = [float(e["att"][0]) for e in res["history"]]
    assert [round(k - a, 6) for k, a in zip(keys, att)][:3] == [w, 2 * w, 0.0]


@pytest.mark.parametrize("phrases,path,want", [
    ([[1, 2, 3], [2, 3, 4]], (1, 2, 3, 4), 6.0),                    # overlapping phrases: both occurrences count
    ([[1, 2], [1, 2, 3]], (1, 2, 4), 2.0),                          # a phrase that is a prefix of another: kept when the longer fails
    ([[1, 2], [1, 2, 3]], (1, 2, 3), None),                         # ... and the longer one completed: walk's value
    ([[3]], (3, 3, 1), 2.0),                                        # a single-token phrase, twice
])
def test_phrase_shapes(phrases, path, want):
    V = 6
    rows = [{t: 0.9} for t in path] + [{V - 1: 0.9}]
    g = ContextGraph(phrases, V, score=1.0)
    res = _run(_table(V, rows), V, 8, 1, 1, [g])
    h = res["nbest"][0]
    assert h[0] == path and h[4]
    assert h[6] == h[7] == g.walk(path)[2]
    if want is not None:
        assert h[6] == want
    for i, e in enumerate(res["history"][:len(path)]):
        assert (e["ctx_state"][0], e["bonus"][0]) == g.walk(path[:i + 1])[:2]


def test_a_hotword_outside_the_pre_beam_is_not_rescued():
    V = 6
    f = _table(V, [{1: 0.5, 2: 0.3, 3: 0.1}, {V - 1: 0.9}])
    g = ContextGraph([[3]], V, score=50.0)
    assert all(3 not in h[0] for h in _run(f, V, 3, 2, 2, [g])["nbest"])
    wide = _run(f, V, 3, 2, 3, [g])
    assert wide["nbest"][wide["best"]][0] == (3,)


def test_at_the_step_limit_the_provisional_credit_stays_in_the_key():
    V, w = 6, 2.0
    g = ContextGraph([[1, 2, 3]], V, score=w)
    res = _run(_table(V, [{1: 0.9}, {2: 0.9}, {3: 0.9}]), V, 2, 1, 1, [g])
    h = res["nbest"][0]
    assert h[0] == (1, 2) and not h[4] and h[6] == 2 * w and h[7] == 0.0 and res["ctx_state"] == [2]
    assert abs(h[1] - (h[2] + 2 * w)) < 1e-12


# ---------------------------------------------------------------------------------------------------------- 4. invariants
def _toy_logp(V, seed):
    def logp_of(tokens):
        g = torch.Generator().manual_seed(hash((seed,) + tuple(tokens)) % (2 ** 31))
        z = torch.randn(V, generator=g, dtype=torch.float64)
        z[V - 1] += 0.8 * len(tokens) - 1.5          # hypotheses end, sooner or later
        return torch.log_softmax(z, dim=-1)
    return logp_of


def test_beam_one_is_greedy_attention_with_the_bonus_accumulated():
    V, m = 7, 9
    g = ContextGraph(cases.random_phrases(V, 6, 3, 1, 3), V, score=0.5)
    logp_of = _toy_logp(V, 3)
    res = _run(logp_of, V, m, 1, 1, [g])
    tokens, att, st, bonus = [], 0.0, 0, 0.0
    for _ in range(m):
        lp = logp_of(tokens)
        c = int(torch.sort(lp, descending=True, stable=True)[1][0])
        tokens.append(c)
        att += float(lp[c])
        if c == V - 1:
            bonus -= float(g.pot[st])
            st = 0
            break
        bonus += float(g.delta[st, g.cls[c]])
        st = int(g.next[st, g.cls[c]])
    (got, key, a, c, fin, _, b, f), = res["nbest"]
    assert got == tuple(t for t in tokens if t != V - 1) and fin == (tokens[-1] == V - 1)
    assert abs(a - att) <= 1e-12 and b == bonus and res["ctx_state"] == [st]
    assert abs(key - (att + float(torch.tensor(bonus, dtype=torch.float32)))) <= 1e-10


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_lock_step_batch_equals_every_utterance_alone(w):
    V, N, P = 6, 3, 4
    ms = [7, 3, 1, 12]
    lm = aed_lm_cases.NgramLm(aed_lm_cases.lm_grams(V, 3, 4, 10, 1)[1], V)
    graphs = [ContextGraph(cases.random_phrases(V, 4, s, 1, 3), V, score=1.0) for s in (1, 2)]

    def ctc(m, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.log_softmax(torch.randn(m, V, generator=g, dtype=torch.float64) * 1.5, dim=-1)

    xs = [ctc(m, 20 + i) if w > 0 else None for i, m in enumerate(ms)]
    fs = [_toy_logp(V, 40 + i) for i in range(len(ms))]
    ids, on = [0, -1, 1, 0], [1, 1, 0, 1]
    batch = ref.search_with(xs, fs, ms, N, P, w, lm, 0.5, 0.5, V - 1, graphs, ids, lm_on=on, extra_steps=3)
    for b in range(len(ms)):
        alone = ref.search_with(xs[b:b + 1], fs[b:b + 1], ms[b:b + 1], N, P, w, lm, 0.5, 0.5, V - 1, graphs, ids[b:b + 1], lm_on=on[b:b + 1])[0]
        for k in ("nbest", "steps", "margin", "lm_state", "n", "ctx_state", "bonus", "final"):
            assert alone[k] == batch[b][k], (b, k)


# ---------------------------------------------------------------------------------------------------- 5. the cases' conditions
@pytest.mark.parametrize("name", list(cases.SPECS))
def test_case_conditions(name):
    """every utterance's float64 margin exceeds twice the yardstick's bound, and the case shows what it exists for"""
    r64, e32, bound = cases.reference(name)
    dcfg, _, _, mem_len, _, spec, lm, graphs = cases.case(name)
    for b, r in enumerate(r64):
        print("aed ctx %s utterance %d: e32 %.3e, bound %.3e, margin %.3e, steps %d / limit %d, final %s" % (
            name, b, e32, bound, r["margin"], r["steps"], r["limit"], r["final"]))
        assert r["margin"] > 2 * bound
    assert all(float(s["score"]) == float(torch.tensor(s["score"], dtype=torch.float32)) for s in spec["graphs"])
    ids = spec["ids"] or [0] * len(mem_len)
    biased = [b for b, g in enumerate(ids) if 0 <= g < len(graphs)]
    assert any(x != 0.0 for b in biased for x in cases.kept_bonus(r64[b]))                 # the context is felt
    ub = cases.unbiased(name)
    assert any(r64[b]["nbest"] != ub[b]["nbest"] for b in biased)
    if name in ("tiny", "ctc", "lm", "att"):
        assert (spec["w"] > 0, lm is not None) == {"tiny": (True, True), "ctc": (True, False), "lm": (False, True), "att": (False, False)}[name]
        assert list(spec["mem"]) == [5, 9, 1] and spec["beam"] == 3 and spec["pre_beam"] == 5 and dcfg.vocab == 11
    if name == "tiny":
        assert any(cases.ancestry_steps(r) and min(cases.ancestry_steps(r)) < len(r["history"]) for r in r64)
    if name == "beam1":
        assert spec["beam"] == 1 and spec["pre_beam"] == 2
    if name == "w1_p_is_vocab":
        assert spec["w"] == 1.0 and spec["pre_beam"] == dcfg.vocab == 5
    if name == "p64":
        assert spec["pre_beam"] == 64 and dcfg.vocab == 70
    if name == "frames":
        assert list(spec["mem"]) == [63, 64, 65] and [r["limit"] for r in r64] == [6, 6, 6]
    if name == "mixed":
        assert len(graphs) == 2 and sorted(ids) == [-1, 0, 1, 2]
        for b in (1, 3):
            assert r64[b]["nbest"] == ub[b]["nbest"] and all(x == 0.0 for x in cases.kept_bonus(r64[b]))
    if name == "graphs":
        g = graphs[0]
        assert any(tuple(q[:len(p)]) == tuple(p) and p != q for p in g.phrases for q in g.phrases)      # a prefix phrase
        assert any(len(p) == 1 for p in g.phrases)
        # a failure link that is taken: from inside (1, 2, 3) the token 4 lands inside (2, 3, 4), not at the start
        s3 = g.walk([1, 2, 3])[0]
        assert g.walk([1, 2, 3, 4])[0] == g.walk([2, 3, 4])[0] != 0 and s3 != 0
        assert sum(cases.retractions(r)[0] + cases.retractions(r)[1] for r in r64) >= 1
    if name == "real":
        assert dcfg.vocab == 1434 and len(graphs[0].phrases) == 50


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_attention_beam_search_refuses_before_it_touches_a_device():
    """a set on the host; and, given a set that claims to be on the device, a wrong vocabulary and a phrase holding eos"""
    from m3asr import _lib
    from m3asr.aed_search import AttentionBeamSearch
    from m3asr.config import DecoderConfig
    dcfg = DecoderConfig.tiny(vocab=11)
    rescorer = types.SimpleNamespace(cfg=dcfg, device="cuda:0")
    on_device = types.SimpleNamespace(is_cuda=True, device=torch.device("cuda:0"))
    host = ContextSet([ContextGraph([[1, 2]], 11)])
    assert host.dev is None
    with pytest.raises(_lib.M3Error, match="not on"):
        AttentionBeamSearch(rescorer, 2, 3, 5, context=host)
    other = ContextSet([ContextGraph([[1, 2]], 12)])
    other.dev = on_device
    with pytest.raises(_lib.M3Error, match="vocabulary of 12"):
        AttentionBeamSearch(rescorer, 2, 3, 5, context=other)
    with_eos = ContextSet([ContextGraph([[1, 2]], 11), ContextGraph([[3, 10]], 11)])
    with_eos.dev = on_device
    with pytest.raises(_lib.M3Error, match="graph 1 .* eos"):
        AttentionBeamSearch(rescorer, 2, 3, 5, context=with_eos)


# -------------------------------------------------------------------------------------------------------------- 7. the ABI
NEW_EXPORTS = ["m3_aed_bias_prune", "m3_aed_bias_reset", "m3_aed_bias_result", "m3_aed_bias_score", "m3_aed_bias_scratch_size",
               "m3_aed_bias_state_size"]


def test_new_exports_and_unchanged_abi_version():
    from m3asr import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m3asr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(m3_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(n for n in declared if n.startswith("m3_aed_bias")) == NEW_EXPORTS
    assert not any("_lm" in n for n in NEW_EXPORTS)
    assert _lib.load().m3_abi_version() == 10
    # the sizes are host arithmetic over B, beam and pre_beam alone
    sdesc = ops.aed_search_desc(3, 3, 9, 11, 32, 2, 2, 100)
    d = ops.aed_bias_desc(sdesc, 5)
    assert ops.aed_bias_state_size(d) == 256 * -(-(3 * 3 * 2 * 16) // 256)
    assert ops.aed_bias_scratch_size(d) == 256 * -(-(3 * 3 * 5 * 32) // 256)
    assert ops.aed_bias_state_size(ops.aed_bias_desc(sdesc, 5, 64)) == ops.aed_bias_state_size(d)
    for p in (2, 65, 12):
        with pytest.raises(_lib.M3Error, match="pre_beam"):
            ops.aed_bias_desc(sdesc, p)
