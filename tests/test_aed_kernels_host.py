"""The mirrors of tests/aed_kernels_ref.py against the contract restatements they stand in for (aed_ref, aed_search_ref), and
the margin / exact-tie condition of every synthetic case tests/test_aed_kernels_gpu.py runs.  No GPU, no library."""
import math

import pytest
import torch

import aed_kernels_ref as kref
import aed_ref
import aed_search_ref as sref


def test_attention_mirror_equals_aed_ref():
    """a packed batch with causal and non-causal slots: per slot aed_ref.attention (identity q / k / out projections, a random
    value projection) on the slot's own rows"""
    H, dk = 2, 16
    D = H * dk
    g = torch.Generator().manual_seed(0)
    q = torch.randn(40, D, generator=g, dtype=torch.float64)
    key = torch.randn(50, D, generator=g, dtype=torch.float64)
    wv = torch.randn(D, D, generator=g, dtype=torch.float64)
    eye, zero = torch.eye(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    sd = {"a.linear_%s.weight" % n: eye for n in "qk"}
    sd.update({"a.linear_out.weight": eye, "a.linear_v.weight": wv})
    sd.update({"a.linear_%s.bias" % n: zero for n in ("q", "k", "v", "out")})
    desc = [(0, 7, 3, 20, 0), (7, 17, 25, 17, 1), (30, 1, 0, 1, 0), (31, 9, 3, 20, 0), (24, 3, 40, 0, 0), (27, 0, 0, 5, 0)]
    out, wrote = kref.attention(q, key, key @ wv.t(), desc, H)
    want_wrote = torch.zeros(40, dtype=torch.bool)
    for q0, n_q, k0, n_k, causal in desc[:4]:
        visible = torch.tril(torch.ones(n_q, n_k, dtype=torch.bool)) if causal else torch.ones(n_q, n_k, dtype=torch.bool)
        want = aed_ref.attention(sd, "a.", H, q[q0:q0 + n_q], key[k0:k0 + n_k], visible)
        assert float((out[q0:q0 + n_q] - want).abs().max()) < 1e-12
        want_wrote[q0:q0 + n_q] = True
    assert torch.equal(wrote, want_wrote) and bool((out[~wrote] == 0).all())


def test_attention_case_layout():
    """the slots of the issue are all there, no two live slots share a query row, and the skip slots' rows belong to nobody"""
    c = kref.attention_case(2, 16)
    assert [tuple(d[1:2] + d[3:]) for d in c["desc"][:8]] == kref.ATT_SLOTS
    assert c["max_q"] > max(d[1] for d in c["desc"])
    owner = torch.zeros(c["q_rows"], dtype=torch.int32)
    for s in c["live"]:
        q0, n_q = c["desc"][s][:2]
        owner[q0:q0 + n_q] += 1
    assert int(owner.max()) == 1
    for s, (r0, n) in c["skipped"].items():
        assert int(owner[r0:r0 + n].sum()) == 0
    _, wrote = kref.attention(c["q"].double(), c["k"].double(), c["v"].double(), c["desc"], c["H"])
    assert torch.equal(wrote, owner.bool())
    for a, b in c["twins"]:
        (qa, na, ka, la, ca), (qb, nb, kb, lb, cb) = c["desc"][a], c["desc"][b]
        assert (na, la, ca) == (nb, lb, cb) and qa != qb and ka != kb and (qa - qb) % 16 != 0
        assert torch.equal(c["q"][qa:qa + na], c["q"][qb:qb + nb]) and torch.equal(c["k"][ka:ka + la], c["k"][kb:kb + lb])
        assert torch.equal(c["v"][ka:ka + la], c["v"][kb:kb + lb])


def test_self_attention_mirror_follows_the_ancestry():
    """A 70-step synthetic search whose K | V rows are a function of the hypothesis's token prefix alone.  The mirror (rows
    fetched through the parents of the history) must equal plain attention over each hypothesis's own prefix, recomputed."""
    case = kref.walk_case(2, 70)
    N, H, dk = case["beam"], 2, 16
    D = H * dk
    trace = kref.run_search(case, torch.float64)
    g = torch.Generator().manual_seed(9)
    memo = {}

    def kv_of(u, prefix):
        if (u, prefix) not in memo:
            memo[(u, prefix)] = torch.randn(2 * D, generator=g, dtype=torch.float64)
        return memo[(u, prefix)]

    kv_steps = []
    for s in range(70):
        kv_steps.append(torch.stack([kv_of(u, tuple(trace[s][u]["tokens"][j])) for u in range(case["B"]) for j in range(N)]))
        if s not in (0, 1, 5, 63, 64, 65, 69):
            continue
        q = torch.randn(case["B"] * N, D, generator=g, dtype=torch.float64)
        out = kref.search_self_attention(q, kv_steps, [trace[s][u]["history"] for u in range(case["B"])], s, N, H)
        for r in range(case["B"] * N):
            u, j = divmod(r, N)
            y = tuple(trace[s][u]["tokens"][j])
            kv = torch.stack([kv_of(u, y[:t]) for t in range(s + 1)])
            for h in range(H):
                c = slice(h * dk, (h + 1) * dk)
                want = torch.softmax(kv[:, c] @ q[r, c] / math.sqrt(dk), 0) @ kv[:, D:][:, c]
                assert float((out[r, c] - want).abs().max()) < 1e-12, (s, r, h)


def _search_cases():
    cases = [kref.search_case(b, v) for b, v in kref.SEARCH_SHAPES]
    cases += [kref.tie_case(), kref.nonfinite_case(), kref.walk_case(2, 5), kref.walk_case(1, 70), kref.walk_case(2, 70),
              kref.walk_case(2, 5, mem_len=(3, 9))]
    return cases


@pytest.mark.parametrize("case", _search_cases(), ids=lambda c: c["name"] + "_" + "_".join(map(str, c["mem_len"])))
def test_synthetic_case_margins(case):
    """every decision of the case is decided by more than twice the bound or is an exact tie by construction, in float64 and
    in float32, and the two precisions take the same decisions"""
    t64, t32 = kref.run_search(case, torch.float64), kref.run_search(case, torch.float32)
    e32, bound = kref.yardstick(kref.search_scores(t64), kref.search_scores(t32))
    m64, ties64 = kref.search_margin(case, t64)
    m32, ties32 = kref.search_margin(case, t32)
    f64 = kref.final_margin(t64)
    print("%s: e32 %.3e, bound %.3e, margin %.3e (float32 %.3e), best margin %.3e, exact ties %d" % (
        case["name"], e32, bound, m64, m32, f64, ties64))
    assert kref.same_discrete(t64, t32)
    assert m64 > 2 * bound and m32 > 2 * bound and f64 > 2 * bound and ties64 == ties32


def test_cases_reach_what_they_are_for():
    eos = 10
    t = kref.run_search(kref.tie_case(), torch.float64)
    assert t[1][0]["tokens"][:2] == [[2], [5]] and float(t[1][0]["score"][0]) == float(t[1][0]["score"][1])
    assert t[2][0]["history"][1]["parent"] == [0, 1, 0] and t[2][0]["tokens"][:2] == [[2, 4], [5, 4]]
    assert float(t[2][0]["score"][0]) == float(t[2][0]["score"][1]) and sref.result(t[2][0], eos)["best"] == 0
    assert kref.search_margin(kref.tie_case(), t)[1] >= 3
    for beam, V in kref.SEARCH_SHAPES:
        case = kref.search_case(beam, V)
        last = kref.run_search(case, torch.float64)[-1]
        assert [s["steps"] for s in last][0] == 1 and all(s["done"] for s in last)
        if V > 1 and beam < V:
            assert last[1]["steps"] == 3 and all(last[1]["finished"]), "utterance 1: every slot finished before the limit 4"
            assert last[2]["steps"] == 7 and not all(last[2]["finished"]), "utterance 2: stopped by the limit of the reset"
            assert beam == 1 or any(e["finished"][j] for e in last[2]["history"][:-1] for j in range(beam)), "no finished row"
    for case in (kref.walk_case(2, 5), kref.walk_case(1, 70), kref.walk_case(2, 70)):
        last = kref.run_search(case, torch.float64)[-1]
        for st in last:
            assert st["steps"] == case["max_steps"] and not any(st["finished"])
            ident = list(range(case["beam"]))
            same = sum(e["parent"] == ident for e in st["history"])       # the short case: no step; the long ones: few
            assert same == 0 if case["max_steps"] == 5 else 4 * same < case["max_steps"], "%d steps with the identity ancestry" % same
            assert any(len(set(e["parent"])) < case["beam"] for e in st["history"][1:]), "no duplicated parent"
    last = kref.run_search(kref.walk_case(2, 5, mem_len=(3, 9)), torch.float64)[-1]
    assert [s["steps"] for s in last] == [3, 5]


def test_nonfinite_mirror_agrees_with_advance():
    """on inputs aed_search_ref.advance accepts, the small mirror of the header's pick order is the same step"""
    for case in (kref.search_case(3, 11), kref.search_case(5, 5), kref.search_case(4, 64), kref.tie_case()):
        a = kref.run_search(case, torch.float64)
        b = kref.run_search(dict(case, nonfinite=True), torch.float64)
        assert kref.same_discrete(a, b)
        assert [[e["parent"] for e in s["history"]] for s in a[-1]] == [[e["parent"] for e in s["history"]] for s in b[-1]]
        sa, sb = kref.search_scores(a), kref.search_scores(b)
        assert torch.equal(torch.isfinite(sa), torch.isfinite(sb)) and float((sa - sb)[torch.isfinite(sa)].abs().max()) < 1e-12


def test_nonfinite_case_picks():
    """the non-finite case does what its docstring says, by the small mirror"""
    case = kref.nonfinite_case()
    t = kref.run_search(case, torch.float64)
    u0 = t[1][0]
    assert u0["tokens"] == [[0], [4], [1]] and u0["finished"] == [False, True, False] and float(u0["score"][2]) == -kref.INF
    u1 = t[1][1]
    assert u1["history"][0]["parent"] == [1, 1, 1] and bool((u1["score"] == -kref.INF).all())
    u2 = t[2][2]
    assert u2["history"][1]["parent"] == [2, 2, 2] and bool(torch.isfinite(u2["score"]).all())
    assert bool(torch.isfinite(t[2][3]["score"]).all())
