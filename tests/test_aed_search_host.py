"""CPU cross-checks of tests/aed_search_ref.py, the restatement that attention decoding on the device is held to
(tests/test_aed_search_gpu.py): beam 1 is greedy decoding, the two-stage top-k is the global top N of the pooled candidates,
a batch in lock step gives every utterance what it gets alone (frozen utterances), the limits, and that the shared test cases
(tests/aed_search_cases.py) show what they were picked for."""
import pytest
import torch

import aed_ref
import aed_search_cases as cases
import aed_search_ref as ref


def _greedy(sd, dcfg, mem, limit):
    """argmax decoding, written without the search: extend by the most probable token until eos or the limit"""
    eos = dcfg.vocab - 1
    sd = {k: v.double() for k, v in sd.items()}
    y, score, finished = [], 0.0, False
    for _ in range(limit):
        logp = aed_ref.decoder_logp(sd, "decoder.", dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + y, mem.double())[-1]
        tok = int(torch.argmax(logp))
        score += float(logp[tok])
        if tok == eos:
            finished = True
            break
        y.append(tok)
    return tuple(y), score, finished


def test_beam_one_is_greedy_decoding():
    dcfg, sd, memory, mem_len, beam, max_steps = cases.case("beam1")
    assert beam == 1
    r64, _, _ = cases.reference("beam1")
    for b, res in enumerate(r64):
        y, score, finished = _greedy(sd, dcfg, memory[b, :mem_len[b]], ref.limit_of(dcfg, mem_len[b], max_steps))
        (tokens, s, f), = res["nbest"]
        assert tokens == y and f == finished and abs(s - score) < 1e-12 and res["best"] == 0
    assert any(cases.stops_early(r) for r in r64) and any(cases.hits_limit_unfinished(r) for r in r64)


def test_two_stage_topk_is_the_global_top_n():
    """every step's kept scores are the N largest of the pool the margin is taken over, in order"""
    dcfg, sd, memory, mem_len, beam, _ = cases.case("tiny")
    eos = dcfg.vocab - 1
    sd64 = {k: v.double() for k, v in sd.items()}
    r64, _, _ = cases.reference("tiny")
    for b, res in enumerate(r64):
        mem = memory[b, :mem_len[b]].double()
        prev = dict(tokens=[[] for _ in range(beam)], score=[0.0] + [-ref.INF] * (beam - 1), finished=[False] * beam)
        for entry in res["history"]:
            pool = []
            for y, s, f in zip(prev["tokens"], prev["score"], prev["finished"]):
                if f:
                    pool.append(s)
                elif s > -ref.INF:
                    logp = aed_ref.decoder_logp(sd64, "decoder.", dcfg.heads, dcfg.num_blocks, dcfg.activation, [eos] + y, mem)[-1]
                    pool += [s + float(v) for v in logp]
            pool.sort(reverse=True)
            assert [float(v) for v in entry["score"]] == pytest.approx(pool[:beam], abs=1e-12)
            gaps = [a - c for a, c in zip(pool[:beam], pool[1:beam + 1])]
            assert res["margin"] <= min(gaps) + 1e-15
            prev = dict(tokens=entry["tokens"], score=[float(v) for v in entry["score"]], finished=entry["finished"])


@pytest.mark.parametrize("name", ["tiny", "tiny_cap4", "beam_is_vocab"])
def test_frozen_utterances(name):
    """the lock-step batch == every utterance alone == the batch stepped three more times"""
    dcfg, sd, memory, mem_len, beam, max_steps = cases.case(name)
    r64, _, _ = cases.reference(name)
    more = ref.search(sd, dcfg, memory, mem_len, beam, max_steps, extra_steps=3)
    for b, res in enumerate(r64):
        alone, = ref.search(sd, dcfg, memory[b:b + 1], mem_len[b:b + 1], beam, max_steps)
        for other in (alone, more[b]):
            assert other["nbest"] == res["nbest"] and other["best"] == res["best"] and other["steps"] == res["steps"]
            assert other["margin"] == res["margin"]
        assert res["steps"] <= res["limit"] == ref.limit_of(dcfg, mem_len[b], max_steps)


def test_limits():
    dcfg = cases.case("tiny")[0]
    assert ref.limit_of(dcfg, 7) == 7 and ref.limit_of(dcfg, 7, 4) == 4 and ref.limit_of(dcfg, 10 ** 6) == dcfg.max_len - 1
    assert [r["limit"] for r in cases.reference("tiny")[0]] == [5, 9, 1]
    assert [r["limit"] for r in cases.reference("tiny_cap4")[0]] == [4, 4, 1]
    assert [r["steps"] for r in cases.reference("tiny_cap4")[0]] == [4, 4, 1]       # max_steps is the binding limit


def test_cases_show_what_they_were_picked_for():
    """the eos bias makes test models end: without it nothing finishes, with it the cases show all three endings, several
    steps with finished and live slots side by side, and a pruning step that needs the ancestry table"""
    dcfg, sd, memory, mem_len, beam, _ = cases.case("tiny")
    plain = dict(sd)
    plain["decoder.output_layer.bias"] = sd["decoder.output_layer.bias"].clone()
    plain["decoder.output_layer.bias"][-1] -= cases.SPECS["tiny"]["eos_bias"]
    assert cases.SPECS["tiny"]["eos_bias"] > 0
    unbiased = ref.search(plain, dcfg, memory, mem_len, beam)
    r64, e32, bound = cases.reference("tiny")
    assert sum(sum(f for _, _, f in r["nbest"]) for r in unbiased) < sum(sum(f for _, _, f in r["nbest"]) for r in r64)
    assert cases.hits_limit_unfinished(r64[0]) and cases.coexist_steps(r64[0]) >= 2 and cases.ancestry_steps(r64[0])
    assert cases.stops_early(r64[1]) and cases.coexist_steps(r64[1]) >= 2
    assert r64[2]["limit"] == 1 and r64[2]["steps"] == 1
    for name in ("tiny", "tiny_cap4", "beam1", "beam_is_vocab"):
        r, e32, bound = cases.reference(name)
        print("%s: e32 %.3e, bound %.3e, margins %s" % (name, e32, bound, ["%.3e" % u["margin"] for u in r]))
        assert all(u["margin"] > 2 * bound for u in r), name
        assert all(len(u["nbest"]) == cases.case(name)[4] for u in r)
