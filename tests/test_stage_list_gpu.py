"""Stage lists of the engine, pinned: every stage's (name, kernel, launches, alg_bytes, flops) and the launch count of a matrix
of bindings, compared with tests/golden/stage_lists.json.

The matrix reaches every router form (staged concat GEMM, router kernel, fused `moe_route`, split x-half GEMM), every place the
top-1 / index happens (router kernel's tail, single-work-group gate + index, top-1 then index, inside the expert launch, inside
`moe_route`), the local and the expert-parallel path and the fp8 quantised-row hand-over; the fixture records which of them each
entry reaches and the test asserts that the union still covers them all.  The run-time switches are read once per process, so
every switch setting runs in a child process of its own (this file run as a script), under a time limit.

Recording (writes the fixture; only on purpose): python tests/test_stage_list_gpu.py --record
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3m-asr-inference_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "stage_lists.json")

# models: "t" tiny (D = 32, 4 experts: staged GEMM router only, no 8/16/32/64-expert forms), "m" D = 64 with 16 experts (router
# kernel, self-routing, fused and split route), "q" D = 512 with 16 experts (the fp8 quantised-row hand-over needs D = 512)
MODELS = {
    "t": dict(output_dim=16, attention_dim=32, attention_heads=2, num_blocks=2, embed_heads=2, embed_dim=32, embed_linear_units=64,
              embed_blocks=1, num_experts=4, hidden_units=64),
    "m": dict(output_dim=16, attention_dim=64, attention_heads=2, num_blocks=2, embed_heads=2, embed_dim=64, embed_linear_units=128,
              embed_blocks=1, num_experts=16, hidden_units=128),
    "q": dict(output_dim=16, attention_dim=512, attention_heads=8, num_blocks=2, embed_heads=4, embed_dim=512, embed_linear_units=512,
              embed_blocks=1, num_experts=16, hidden_units=512),
}
SHAPES = {"b1": (1, 100), "long": (64, 300)}     # 24 rows; 64 x 74 = 4736 rows (router kernel, top-1 + index, fused fp8 kernel)
DTYPES = {"f32": dict(weight_dtype="f32"), "bf16": dict(weight_dtype="bf16"), "fp8": dict(weight_dtype="fp8"),
          "fp8a": dict(weight_dtype="fp8", fp8_activations=True)}


def _matrix():
    """[(key, entry)]: entry = dict(model, dtype, shape, fuse_route, packed, fork, taps, ep, stream, env)."""
    out = []

    def add(model, dtype, shape, fuse_route=0, packed=None, fork=None, taps=False, ep=False, stream=False, env=None):
        e = dict(model=model, dtype=dtype, shape=shape, fuse_route=fuse_route, packed=packed, fork=fork, taps=taps, ep=ep,
                 stream=stream, env=env or {})
        key = "%s.%s.%s.r%d" % (model, dtype, shape, fuse_route)
        for k, v in (("packed", packed), ("fork", fork)):
            if v is not None:
                key += ".%s%d" % (k, int(v))
        for k in ("taps", "ep", "stream"):
            if e[k]:
                key += "." + k
        for k, v in sorted(e["env"].items()):
            key += ".%s=%s" % (k, v)
        out.append((key, e))

    for model in ("t", "m"):
        for shape in SHAPES:
            for fr in (0, 1, 2):
                add(model, "f32", shape, fr)
            for dt in ("bf16", "fp8", "fp8a") if model == "m" else ("bf16",):     # (fp8 experts need D % 64 == 0)
                add(model, dt, shape)
    for dt in ("fp8", "fp8a"):
        add("q", dt, "long")
    add("q", "fp8a", "b1")
    add("m", "f32", "long", packed=False)
    add("m", "bf16", "long", packed=False)
    add("m", "f32", "b1", packed=True)
    add("m", "f32", "b1", fork=True)
    add("m", "f32", "b1", 1, fork=True)
    add("m", "f32", "b1", fork=False)
    add("m", "f32", "b1", taps=True)
    add("m", "f32", "long", taps=True)
    for dt in ("f32", "bf16", "fp8a"):
        for shape in SHAPES:
            add("m", dt, shape, ep=True)
    add("q", "fp8a", "long", ep=True)
    add("m", "f32", "b1", stream=True)
    # the run-time switches away from their defaults, one child process each
    for fr in (0, 2):
        add("m", "f32", "b1", fr, env={"M3_SELF_ROUTE": "0"})
    add("q", "fp8a", "long", env={"M3_ROUTER_XQ": "0"})
    add("q", "fp8a", "long", env={"M3_ROUTER_SKIP_XN": "1"})
    add("q", "fp8a", "long", env={"M3_FUSED8_ADAPT": "1"})
    for fr in (0, 1):
        add("m", "f32", "b1", fr, env={"M3_HFUSE": "0"})
    for dt, shape in (("bf16", "b1"), ("f32", "long"), ("bf16", "long")):
        add("m", dt, shape, env={"M3_GATE_INDEX_MAX_ROWS": "16"})
    add("m", "bf16", "b1", ep=True, env={"M3_GATE_INDEX_MAX_ROWS": "16"})
    for dt in ("f32", "bf16"):
        add("m", dt, "b1", env={"M3_ROUTER_MIN_ROWS": "16"})
    add("m", "f32", "b1", 2, env={"M3_ROUTER_MIN_ROWS": "16"})
    return out


# The one intended difference from the recording: with fuse_route = 2 and an expert count outside {8, 16, 32, 64} the split route
# is not taken, and the "router_e_all" GEMM (its output read by nobody) is no longer built.
DROPS_ROUTER_E_ALL = {"t.f32.b1.r2"}   # (4 experts, 24 rows; at 4736 rows neither built the GEMM)


def _forms(entry, stages, xn_offered):
    """Which router form / top-1 placement / path the binding's first MoE block took, read off its stage list."""
    from m3asr.config import EncoderConfig, subsampled_len
    cfg = EncoderConfig(**MODELS[entry["model"]])
    names = [s[0] for s in stages]
    blk = {n[len("blocks.0."):]: s for n, s in zip(names, stages) if n.startswith("blocks.0.")}
    if not blk:
        return []
    B, T = SHAPES[entry["shape"]]
    S = B * (4 if entry["stream"] else subsampled_len(T))   # (streaming: one chunk of static_chunk_size = 4 frames)
    f = ["ep" if "moe_ep.send" in blk else "local"]
    if "moe_route" in blk:
        f.append("router:fused")
    elif blk["moe_router"][1] == "moe_router_kernel":
        f.append("router:kernel")
    else:   # the GEMM's K: D (split route's x half) or De + D (staged concat)
        K = blk["moe_router"][4] / (2.0 * S * cfg.num_experts)
        f.append("router:split" if round(K) == cfg.attention_dim else "router:gemm")
    if "moe_route" in blk:
        f.append("gate:in_route")
    elif "moe_gate_index" in blk:
        f.append("gate:gate_index")
    elif "moe_top1" in blk:
        f.append("gate:top1_index")
    elif "moe_local.index" in blk or "moe_ep.send" in blk:
        f.append("gate:router_tail")
    else:
        f.append("gate:in_expert")
    dt = entry["dtype"]
    local_fused8 = "moe_local.expert" in blk and blk["moe_local.expert"][1] == "expert_ffn_fused_fp8_kernel"
    if dt == "fp8a" and local_fused8 and "router:kernel" in f and entry["env"].get("M3_ROUTER_XQ", "1") != "0":
        f.append("xq")
    if not xn_offered:
        f.append("xn_skipped")
    if dt == "fp8a" and local_fused8 and entry["env"].get("M3_FUSED8_ADAPT", "0") != "0":
        f.append("fs_dev")
    if "router_e_all" in names:
        f.append("e_all")
    return f


def _bind(entry):
    """Build and bind one matrix entry on cuda:0; returns (stages, num_kernels, forms)."""
    import torch
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    kw = dict(MODELS[entry["model"]], **DTYPES[entry["dtype"]])
    if entry["stream"]:
        kw.update(causal=True, embed_causal=True, static_chunk_size=4)
    cfg = EncoderConfig(**kw)
    w = make_weights(cfg, seed=1)
    eng = Engine.from_state_dict(cfg, w, fuse_route=entry["fuse_route"], packed_rows=entry["packed"],
                                 fork_embed=entry["fork"], debug_taps=entry["taps"], ep_stages=entry["ep"])
    B, T = SHAPES[entry["shape"]]
    if entry["stream"]:
        st = eng.streaming(B, 16)
        st.step(torch.zeros(B, st.window, cfg.input_dim, device="cuda:0"), torch.full((B,), st.window, dtype=torch.int32),
                use_graph=False)
        torch.cuda.synchronize()
    else:
        eng.bind(torch.zeros(B, T, cfg.input_dim, device="cuda:0"), torch.full((1, B), T, dtype=torch.int32, device="cuda:0"))
    stages = [[s["name"], s["kernel"], s["launches"], s["alg_bytes"], s["flops"]] for s in eng.stage_info()]
    try:
        st.buffer("xn") if entry["stream"] else eng.buffer("xn")
        xn_offered = True
    except Exception:
        xn_offered = False
    return stages, eng.num_kernels(), _forms(entry, stages, xn_offered)


def _child(env_key):
    """Every matrix entry whose switch setting is `env_key` (a JSON dict), bound in this process: one JSON line on stdout."""
    want = json.loads(env_key)
    res = {}
    for key, entry in _matrix():
        if entry["env"] == want:
            stages, nk, forms = _bind(entry)
            res[key] = dict(stages=stages, num_kernels=nk, forms=forms)
    print("STAGE_LISTS " + json.dumps(res))


def _run_all():
    """The whole matrix, one fresh child process per switch setting (switches are read once per process)."""
    groups = []
    for _, e in _matrix():
        k = json.dumps(e["env"], sort_keys=True)
        if k not in groups:
            groups.append(k)
    base = {k: v for k, v in os.environ.items() if not k.startswith("M3_")}
    res = {}
    for i, k in enumerate(groups):
        print("stage lists: switch setting %d/%d %s" % (i + 1, len(groups), k), file=sys.stderr, flush=True)
        env = dict(base, **json.loads(k))
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", k], env=env,
                           cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 0, "stage-list child %s exited with %d:\n%s" % (k, p.returncode, p.stderr[-4000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("STAGE_LISTS ")][-1]
        res.update(json.loads(line[len("STAGE_LISTS "):]))
    return res


REQUIRED_FORMS = {"local", "ep", "router:gemm", "router:kernel", "router:fused", "router:split", "gate:router_tail",
                  "gate:gate_index", "gate:top1_index", "gate:in_expert", "gate:in_route", "xq", "xn_skipped", "fs_dev", "e_all"}


@pytest.mark.gpu
def test_stage_lists_match_fixture():
    with open(FIXTURE) as fh:
        want = json.load(fh)
    keys = [k for k, _ in _matrix()]
    assert sorted(want) == sorted(keys), "the matrix and the fixture name different bindings"
    covered = set().union(*(set(v["forms"]) for v in want.values()))
    assert REQUIRED_FORMS <= covered, "the fixture no longer reaches %s" % sorted(REQUIRED_FORMS - covered)
    got = _run_all()
    for k in keys:
        w = want[k]
        exp_stages, exp_nk = w["stages"], w["num_kernels"]
        exp_forms = w["forms"]
        if k in DROPS_ROUTER_E_ALL:
            assert [s[0] for s in exp_stages].count("router_e_all") == 1
            exp_nk -= [s[2] for s in exp_stages if s[0] == "router_e_all"][0]
            exp_stages = [s for s in exp_stages if s[0] != "router_e_all"]
            exp_forms = [f for f in exp_forms if f != "e_all"]
        assert got[k]["stages"] == exp_stages, "stage list of %s differs" % k
        assert got[k]["num_kernels"] == exp_nk, "num_kernels of %s differs" % k
        assert got[k]["forms"] == exp_forms, "%s reaches %s, recorded %s" % (k, got[k]["forms"], exp_forms)


if __name__ == "__main__":
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    elif sys.argv[1:] == ["--record"]:
        data = _run_all()
        with open(FIXTURE, "w") as fh:
            json.dump(data, fh, sort_keys=True, separators=(",", ":"))
            fh.write("\n")
        print("recorded %d bindings into %s" % (len(data), FIXTURE))
    else:
        sys.exit("usage: test_stage_list_gpu.py --record | --child ENV_JSON")
