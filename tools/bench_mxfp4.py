#!/usr/bin/env python3
"""The expert weights in bf16, fp8 and mxfp4 side by side: plan bytes and forward time.

  python tools/bench_mxfp4.py [--layers 18] [--experts 32] [--dtypes bf16,fp8,mxfp4] [--repeats 7] [--steps 100] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_mxfp4.py --kernel-only [--dtypes fp8,mxfp4] [--steps 200]

(bench.py's --weight-dtype choices are fixed, so the 4-bit mode is measured here.)  Builds the synthetic 18-layer x 32-expert
model once (seeded weights and features) and, for every dtype, an engine on the same weights.  Per dtype one JSON line:
  * plan_bytes: the bytes of the packed tensors (what save_plan writes, without its 256-byte padding), and the expert share;
  * ms at 1 x 206 frames and at 16 x 50-500 frames (lengths drawn once from U[50, 500], the longest 500): hipGraph replays,
    --steps forwards between two stream synchronisations under a host clock, --repeats such windows after a warm-up of one
    window per shape, the dtypes ALTERNATING inside every repeat (other work shares the host: a drift then hits all of them);
    reported: the median window and the min / max, as ms per forward;
  * the kernel the expert stage runs at each shape (the plan's label).
--kernel-only: no timing; per dtype --steps graph replays of the 1 x 206 forward and nothing else, for a kernel trace in a run
of its own (the expert kernel's time per launch is the trace's figure for expert_ffn_w8_kernel / expert_ffn_w4_kernel).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))
import numpy as np
import torch

from m3asr.config import EncoderConfig
from m3asr.engine import Engine
from m3asr.plan import pack_weights
from m3asr.weights import make_weights


def plan_bytes(packed):
    total = sum(v.numel() * v.element_size() for v in packed.values())
    experts = sum(v.numel() * v.element_size() for k, v in packed.items()
                  if ".experts.w_" in k and (k.endswith("weight") or k.endswith("weight_sliced") or k.endswith("scale")))
    return total, experts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--experts", type=int, default=32)
    ap.add_argument("--dtypes", default="bf16,fp8,mxfp4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mxfp4: needs a GPU (nothing here is measured without one)")
    dtypes = args.dtypes.split(",")
    base = EncoderConfig(num_blocks=args.layers, num_experts=args.experts)
    weights = make_weights(base, seed=7)
    rng = np.random.default_rng(1234)
    lengths = rng.integers(50, 501, 16)
    lengths[0] = 500
    shapes = {"1x206": (torch.from_numpy(rng.random((1, 206, base.input_dim), dtype=np.float32)), np.array([206])),
              "16x50-500": (torch.from_numpy(rng.random((16, 500, base.input_dim), dtype=np.float32)), lengths)}
    if args.kernel_only:
        shapes = {"1x206": shapes["1x206"]}

    info, ctx = {}, {}
    for dt in dtypes:
        cfg = EncoderConfig(**{**base.__dict__, "weight_dtype": dt})
        packed = pack_weights(weights, cfg)
        total, experts = plan_bytes(packed)
        eng = Engine(cfg, packed)
        info[dt] = {"weight_dtype": dt, "layers": args.layers, "experts": args.experts, "plan_bytes": total, "expert_bytes": experts,
                    "shapes": {}}
        del packed
        for name, (feat, lens) in shapes.items():
            c = eng if not ctx.get(dt) else eng.clone_context()       # one context (stream, workspace, graph) per shape
            c.bind(feat.cuda(), torch.from_numpy(lens.astype(np.int32)).view(1, -1).cuda())
            c.forward(use_graph=False)
            c.stream.synchronize()
            kern = {s_["name"]: s_["kernel"] for s_ in c.stage_info()}
            info[dt]["shapes"][name] = {"frames": int(lens.sum()), "expert_kernel": kern.get("blocks.0.moe_local.expert")}
            ctx.setdefault(dt, {})[name] = c

    def window(c, n):
        c.stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            c.forward(use_graph=True)
        c.stream.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    if args.kernel_only:
        for dt in dtypes:
            window(ctx[dt]["1x206"], args.steps)
        print(json.dumps({"kernel_only": True, "steps": args.steps, "dtypes": dtypes}))
        return
    for name in shapes:                              # warm-up: capture + one window per (dtype, shape)
        for dt in dtypes:
            window(ctx[dt][name], args.steps)
    samples = {(dt, name): [] for dt in dtypes for name in shapes}
    for _ in range(args.repeats):
        for name in shapes:
            for dt in dtypes:                        # alternating: every repeat visits every dtype
                samples[(dt, name)].append(window(ctx[dt][name], args.steps))
    for dt in dtypes:
        for name in shapes:
            s = np.array(samples[(dt, name)])
            d = info[dt]["shapes"][name]
            d.update(ms_median=round(float(np.median(s)), 4), ms_min=round(float(s.min()), 4), ms_max=round(float(s.max()), 4),
                     frames_per_s=round(d["frames"] / (float(np.median(s)) * 1e-3), 1))
        info[dt].update(steps=args.steps, repeats=args.repeats)
        line = json.dumps(info[dt])
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
