"""CPU checks of tests/aed_lm_ref.py, the restatement that attention decoding with LM fusion on the device is held to
(tests/test_aed_lm_gpu.py): against the joint restatement it extends, against NgramLm.step and the textbook ARPA scorer of
tests/lm_ref.py, and against invariants of the search itself; and the conditions the cases of tests/aed_lm_cases.py were
picked for."""
import pytest
import torch

import aed_joint_cases
import aed_lm_cases as cases
import aed_lm_ref as ref
import lm_ref
from m3asr.lm import NgramLm

INF = float("inf")
SMALL = [n for n in cases.SPECS if n != "real"]


def _lm(V, order=3, unigrams=7, higher=30, seed=1):
    return NgramLm(cases.lm_grams(V, order, unigrams, higher, seed)[1], V)


@pytest.mark.parametrize("how", ["zero_weights", "lm_off"])
def test_without_weights_or_switched_off_it_is_the_joint_search(how):
    """alpha = beta = 0, or lm_on = 0 for every utterance: aed_joint_ref's results on aed_joint_cases' tiny, exactly"""
    dcfg, sd, memory, mem_len, ctc, spec = aed_joint_cases.case("tiny")
    want = aed_joint_cases.reference("tiny")[0]
    alpha, beta, on = (0.0, 0.0, None) if how == "zero_weights" else (0.5, 4.0, [0] * len(mem_len))
    got = ref.search(sd, dcfg, memory, mem_len, ctc, spec["beam"], spec["pre_beam"], spec["w"], _lm(dcfg.vocab), alpha, beta, True, on,
                     spec["max_steps"])
    for g, w in zip(got, want):
        assert [h[:5] for h in g["nbest"]] == w["nbest"] and g["best"] == w["best"]
        assert g["margin"] == w["margin"] and g["steps"] == w["steps"] and g["limit"] == w["limit"]
        for eg, ew in zip(g["history"], w["history"]):
            for k in ("key", "att", "ctc"):
                assert torch.equal(eg[k], ew[k]), k
            assert eg["tokens"] == ew["tokens"] and eg["parent"] == ew["parent"] and eg["flat"] == ew["flat"]
        if how == "lm_off":
            eos = dcfg.vocab - 1                                          # a finished slot repeats eos: n counts up to the first
            assert all(h[5] == 0.0 for h in g["nbest"]) and g["n"] == [t.index(eos) + 1 if eos in t else len(t) for t in g["tokens"]]


@pytest.mark.parametrize("name", SMALL)
def test_lm_part_is_the_sum_of_steps_and_the_textbook_score(name):
    """every final hypothesis: lm == NgramLm.step summed over its tokens plus the eos term, bit for bit in double; and the
    textbook scorer of tests/lm_ref.py to the 1e-6 the CTC fusion's tests use; the carried LM state is the re-walked one"""
    dcfg, _, _, _, _, spec, lm, grams10 = cases.case(name)
    eos = dcfg.vocab - 1
    on = spec["lm_on"] or [1] * len(spec["mem"])
    checked = 0
    for b, res in enumerate(cases.reference(name)[0]):
        for toks, h, state, n in zip(res["tokens"], res["nbest"], res["lm_state"], res["n"]):
            y = toks[:toks.index(eos) + 1] if eos in toks else toks
            assert n == len(y)
            if not on[b]:
                assert h[5] == 0.0 and state == lm.start
                continue
            st, total = lm.start, 0.0
            for t in y:
                if t == eos:
                    total = total + float(lm.final[st]) * (1 if spec["use_eos"] else 0)
                else:
                    d, st, _ = lm.step(st, t)
                    total = total + d
            assert h[5] == total and state == st, (toks, h[5], total)
            assert (st, total if not h[4] else total - float(lm.final[st]) * spec["use_eos"]) == lm.walk(h[0])
            want = lm_ref.arpa_score(grams10, h[0], eos=h[4] and spec["use_eos"])
            assert h[5] == pytest.approx(want, abs=1e-6, rel=1e-6), (toks, h[5], want)
            checked += 1
    assert checked >= spec["beam"]


def _toy_logp(V, seed):
    """an attention model that needs no weights: log-probabilities drawn from a generator seeded by the prefix"""
    def logp_of(tokens):
        g = torch.Generator().manual_seed(hash((seed,) + tuple(tokens)) % (2 ** 31))
        z = torch.randn(V, generator=g, dtype=torch.float64)
        z[V - 1] += 0.8 * len(tokens) - 1.5          # hypotheses end, sooner or later
        return torch.log_softmax(z, dim=-1)
    return logp_of


def _ctc(m, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(m, V, generator=g, dtype=torch.float64) * 1.5, dim=-1)


@pytest.mark.parametrize("w", [0.0, 0.4])
def test_beam_one_is_greedy_attention_with_the_lm_part_accumulated(w):
    V, m, alpha, beta = 7, 9, 0.5, 0.25
    lm, logp_of = _lm(V, unigrams=4, higher=10), _toy_logp(V, 3)
    x = _ctc(m, V, 11) if w > 0 else None
    res = ref.search_with([x], [logp_of], [m], 1, 1, w, lm, alpha, beta, V - 1)[0]
    tokens, att, st, total = [], 0.0, lm.start, 0.0
    for _ in range(m):
        lp = logp_of(tokens)
        c = int(torch.sort(lp, descending=True, stable=True)[1][0])
        tokens.append(c)
        att += float(lp[c])
        if c == V - 1:
            total += float(lm.final[st])
            break
        d, st, _ = lm.step(st, c)
        total += d
    (got, key, a, c, fin, l), = res["nbest"]
    assert got == tuple(t for t in tokens if t != V - 1) and fin == (tokens[-1] == V - 1)
    assert abs(a - att) <= 1e-12 and l == total and res["lm_state"] == [st] and res["n"] == [len(tokens)]
    jkey = att if w == 0 else (-INF if c == -INF else (1 - w) * att + w * c)
    assert (key == -INF and jkey == -INF) or abs(key - (jkey + ref.lm_term(alpha, beta, total, len(tokens)))) <= 1e-10


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_lock_step_batch_equals_every_utterance_alone(w):
    V, N, P = 6, 3, 4
    ms = [7, 3, 1, 12]
    lm = _lm(V, unigrams=4, higher=10)
    xs = [_ctc(m, V, 20 + i) if w > 0 else None for i, m in enumerate(ms)]
    fs = [_toy_logp(V, 40 + i) for i in range(len(ms))]
    on = [1, 0, 1, 1]
    batch = ref.search_with(xs, fs, ms, N, P, w, lm, 0.5, 0.5, V - 1, lm_on=on, extra_steps=3)
    for b in range(len(ms)):
        alone = ref.search_with(xs[b:b + 1], fs[b:b + 1], ms[b:b + 1], N, P, w, lm, 0.5, 0.5, V - 1, lm_on=on[b:b + 1])[0]
        for k in ("nbest", "steps", "margin", "lm_state", "n"):
            assert alone[k] == batch[b][k], (b, k)


def test_length_bonus_lengthens_the_shortest_finished_hypothesis():
    """tiny against the same search with beta = 0, over the utterances that can hold more than one token (the third has one
    frame, so its limit is one step and the only hypothesis that can finish there is the empty one): the shortest finished
    hypothesis gets strictly longer, and no utterance's gets shorter"""
    with_bonus, without = cases.reference("tiny")[0], cases.reference("tiny_beta0")[0]
    assert cases.SPECS["tiny"]["beta"] > 0 and cases.SPECS["tiny_beta0"]["beta"] == 0
    assert {k: v for k, v in cases.SPECS["tiny"].items() if k != "beta"} == {k: v for k, v in cases.SPECS["tiny_beta0"].items() if k != "beta"}
    longer = [r["limit"] > 1 for r in without]
    assert longer == [True, True, False]
    a = cases.shortest_finished([r for r, l in zip(without, longer) if l])
    b = cases.shortest_finished([r for r, l in zip(with_bonus, longer) if l])
    print("shortest finished hypothesis: %d tokens without the bonus, %d with it" % (a, b))
    assert a is not None and b is not None and b > a
    for r0, r1 in zip(without, with_bonus):
        assert cases.shortest_finished([r1]) >= cases.shortest_finished([r0])


@pytest.mark.parametrize("name", list(cases.SPECS))
def test_case_conditions(name):
    """every utterance's float64 margin exceeds twice the yardstick's bound, and the case shows what it exists for"""
    r64, e32, bound = cases.reference(name)
    spec = cases.case(name)[5]
    for b, r in enumerate(r64):
        print("aed lm %s utterance %d: e32 %.3e, bound %.3e, margin %.3e, steps %d / limit %d" % (name, b, e32, bound, r["margin"], r["steps"], r["limit"]))
        assert r["margin"] > 2 * bound
    levels = [lv for r in r64 for lv in cases.kept_levels(r)]
    if name == "unigram":
        assert cases.case(name)[6].n_states == 1 and set(levels) == {0}
    if name == "bigram":
        assert cases.case(name)[6].order == 2 and set(levels) == {0, 1}
    if name == "backoff":
        assert max(levels) >= 2 and sum(cases.kept_unknown(r) for r in r64) >= 1
    if name in ("tiny", "mixed"):
        assert any(cases.ancestry_steps(r) and min(cases.ancestry_steps(r)) < len(r["history"]) for r in r64)
        assert cases.case(name)[6].order == 3
    if name == "mixed":
        assert spec["lm_on"] == (1, 0, 1) and all(h[5] == 0.0 for h in r64[1]["nbest"]) and any(h[5] != 0.0 for h in r64[0]["nbest"])
    if name == "w0":
        assert spec["w"] == 0 and all(h[3] == 0.0 and h[1] != h[2] for r in r64 for h in r["nbest"] if h[2] > -INF)
    if name == "p64":
        assert spec["pre_beam"] == 64 and spec["dcfg"].vocab == 70
    if name == "frames":
        assert list(spec["mem"]) == [63, 64, 65] and max(levels) >= 1
    if name == "no_eos":
        assert not spec["use_eos"] and any(h[4] for r in r64 for h in r["nbest"])
    if name == "beta_only":
        assert spec["alpha"] == 0 and spec["beta"] > 0
    if name == "real":
        assert spec["dcfg"].vocab == 1434 and cases.case(name)[6].n_grams > 2000 and max(levels) >= 1
