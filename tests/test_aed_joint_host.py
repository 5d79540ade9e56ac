"""CPU cross-checks of tests/aed_joint_ref.py, the restatement that joint CTC/attention decoding on the device is held to
(tests/test_aed_joint_gpu.py), against three things it shares no code with: a brute-force sum over all alignments,
torch.nn.functional.ctc_loss, and invariants of the search itself."""
import itertools
import math

import numpy as np
import pytest
import torch

import aed_joint_ref as ref

INF = float("inf")


def _logp(m, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(m, V, generator=g, dtype=torch.float64) * 1.5, dim=-1)


def _collapse(path):
    out, prev = [], None
    for s in path:
        if s != prev and s != 0:
            out.append(s)
        prev = s
    return tuple(out)


@pytest.mark.parametrize("m,V,seed", [(1, 3, 0), (2, 4, 1), (3, 3, 2), (4, 4, 3), (5, 3, 4), (5, 4, 5)])
def test_prefix_scores_against_all_alignments(m, V, seed):
    """exp(psi(h)) = the summed probability of the alignments whose collapse BEGINS with h; exp(psi(h . eos)) = of those whose
    collapse IS h: every h up to length 3 over the non-blank, non-eos tokens, repeated tokens and |h| > m (probability 0,
    psi = -inf, no NaN) included.  The CTC vocabulary is the search's: blank 0, eos V - 1, so eos never occurs inside an
    alignment's collapse and its column only takes probability mass away."""
    x = _logp(m, V, seed)
    eos = V - 1
    begins, equals = {}, {}
    for path in itertools.product(range(V), repeat=m):
        p = math.exp(sum(float(x[t, s]) for t, s in enumerate(path)))
        col = _collapse(path)
        equals[col] = equals.get(col, 0.0) + p
        for n in range(len(col) + 1):
            begins[col[:n]] = begins.get(col[:n], 0.0) + p
    tokens = list(range(1, V - 1))
    checked = 0
    for n in range(0, 4):
        for h in itertools.product(tokens, repeat=n):
            psi, state = ref.prefix_score(x, h)
            assert not bool(torch.isnan(psi))
            assert abs(math.exp(float(psi)) - begins.get(h, 0.0)) <= 1e-12, (h, float(psi))
            if n > m:
                assert float(psi) == -INF
            end, _ = ref.prefix_score(x, list(h) + [eos])
            assert not bool(torch.isnan(end))
            assert abs(math.exp(float(end)) - equals.get(h, 0.0)) <= 1e-12, (h, float(end))
            assert not bool(np.isnan(state["rn"]).any() | np.isnan(state["rb"]).any())
            checked += 1
    assert checked >= 1 + len(tokens)
    # a blank inside a hypothesis: probability 0 for it and for everything behind it
    assert float(ref.prefix_score(x, [0])[0]) == -INF and float(ref.prefix_score(x, [0, 1])[0]) == -INF
    assert float(ref.prefix_score(x, [0, eos])[0]) == -INF


@pytest.mark.parametrize("m,V,seed", [(6, 5, 0), (9, 7, 1), (4, 4, 2), (3, 6, 3)])
def test_finished_hypotheses_against_ctc_loss(m, V, seed):
    """ctc(h . eos) == -ctc_loss(h) in float64, reduction "sum": repeated tokens, the empty target, a target that fits exactly,
    and one that cannot be aligned (infinite loss, -inf here)"""
    x = _logp(m, V, seed)
    eos = V - 1
    targets = [[], [1], [1, 1], [2, 1, 2], [1, 2, 2, 1], list(range(1, V - 1)), [1] * m, [1, 1, 1, 1, 1]]
    for h in targets:
        got = float(ref.prefix_score(x, h + [eos])[0])
        loss = torch.nn.functional.ctc_loss(x.unsqueeze(1), torch.tensor([h], dtype=torch.long).reshape(1, -1), torch.tensor([m]),
                                            torch.tensor([len(h)]), blank=0, reduction="sum", zero_infinity=False)
        if math.isinf(float(loss)):
            assert got == -INF, (h, got)
        else:
            assert abs(got + float(loss)) <= 1e-10, (h, got, float(loss))


def _toy_logp(V, seed):
    """an attention model that needs no weights: log-probabilities drawn from a generator seeded by the prefix"""
    def logp_of(tokens):
        g = torch.Generator().manual_seed(hash((seed,) + tuple(tokens)) % (2 ** 31))
        z = torch.randn(V, generator=g, dtype=torch.float64)
        z[V - 1] += 0.8 * len(tokens) - 1.5          # hypotheses end, sooner or later
        return torch.log_softmax(z, dim=-1)
    return logp_of


def test_beam_one_is_greedy_attention_with_the_ctc_part_accumulated():
    V, m, w = 7, 9, 0.4
    x, logp_of = _logp(m, V, 11), _toy_logp(V, 3)
    res = ref.search_with([x], [logp_of], [m], 1, 1, w)[0]
    tokens, att = [], 0.0
    for _ in range(m):
        lp = logp_of(tokens)
        c = int(torch.sort(lp, descending=True, stable=True)[1][0])
        tokens.append(c)
        att += float(lp[c])
        if c == V - 1:
            break
    (got, key, a, c, fin), = res["nbest"]
    assert got == tuple(t for t in tokens if t != V - 1) and fin == (tokens[-1] == V - 1)
    assert abs(a - att) <= 1e-12
    ctc = float(ref.prefix_score(x, tokens)[0])
    assert (c == ctc == -INF) or abs(c - ctc) <= 1e-10
    assert (key == -INF and ctc == -INF) or abs(key - ((1 - w) * att + w * ctc)) <= 1e-10


def test_lock_step_batch_equals_every_utterance_alone():
    V, w, N, P = 6, 0.5, 3, 4
    ms = [7, 3, 1, 12]
    xs = [_logp(m, V, 20 + i) for i, m in enumerate(ms)]
    fs = [_toy_logp(V, 40 + i) for i in range(len(ms))]
    batch = ref.search_with(xs, fs, ms, N, P, w, extra_steps=3)
    for b in range(len(ms)):
        alone = ref.search_with(xs[b:b + 1], fs[b:b + 1], ms[b:b + 1], N, P, w)[0]
        assert alone["nbest"] == batch[b]["nbest"] and alone["steps"] == batch[b]["steps"] and alone["margin"] == batch[b]["margin"]


def test_incremental_states_equal_states_from_scratch():
    """what the search carries through pruning against the scorer run over the final token lists: psi and the whole rn / rb"""
    V, w, N, P = 6, 0.3, 4, 5
    for seed, m in ((1, 8), (2, 5), (3, 13)):
        x, logp_of = _logp(m, V, seed), _toy_logp(V, seed)
        res = ref.search_with([x], [logp_of], [m], N, P, w)[0]
        for toks, (_, key, att, ctc, fin), st in zip(res["tokens"], res["nbest"], res["states"]):
            y = toks[:toks.index(V - 1) + 1] if V - 1 in toks else toks
            psi, state = ref.prefix_score(x, y)
            assert (ctc == float(psi) == -INF) or abs(ctc - float(psi)) <= 1e-10
            if not fin and att > -INF:
                for k in ("rn", "rb"):
                    a, b = st[k], state[k]
                    with np.errstate(invalid="ignore"):
                        same = (a == b) | (np.abs(a - b) <= 1e-10)
                    assert bool(same.all()), (toks, k)


def test_keys_order_candidates_and_minus_inf_keys_order_by_flat_index():
    """m = 2 with beam 3: after two tokens nothing can be extended but by eos, so -inf keys must be kept, in flat-index order"""
    V, N, P = 5, 3, 4
    x, logp_of = _logp(2, V, 5), _toy_logp(V, 9)
    res = ref.search_with([x], [logp_of], [2], N, P, 0.5)[0]
    for e in res["history"]:
        keys = e["key"].tolist()
        assert keys == sorted(keys, reverse=True)
        for a, b, fa, fb in zip(keys[:-1], keys[1:], e["flat"][:-1], e["flat"][1:]):
            if a == b:
                assert fa < fb
        assert not bool(torch.isnan(e["key"]).any() | torch.isnan(e["ctc"]).any())
