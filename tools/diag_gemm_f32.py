"""Phase stamps of the skinny fp32 GEMM at B = 1 shapes (diagnostic build: make EXTRA=-DM3_GEMM_DIAG OBJDIR=build_gdiag
LIB=../tools/_diag_gemm.so; run with M3ASR_LIB=tools/_diag_gemm.so).  Median shader-clock cycles over the work-groups of the LAST
launch: set-up (tile / row descriptors) | issue of the loads | wait for them | MFMAs | LDS reduction + barrier | epilogue | store
drain.  `cold`: rotates through 64 weight matrices (> 256 MB) so that W comes from HBM, as in the 18-layer forward.
`frag`: the weights in MFMA-fragment order (m3_linear_wfrag); `both`: row-major then fragment order in one process.
`mask_out` / `mask_in`: the launch carries a row mask (one utterance of M - 13 frames, rows_per_batch = M), as conv.pw2 / conv.pw1 do.
`router`: instead of a linear, the engine's staged router GEMM on cat([embed, LN(x)]) with the embed prefix (acc_init, ln_out;
no ABI entry reaches that form): a two-block 512-wide, 32-expert engine at 206 frames (50 rows) is run up to block 0's router and
the stamps of that launch's work-groups are read (M N K are ignored).
usage: diag_gemm_f32.py M N K [ln] [cold] [frag | both] [mask_out | mask_in]   |   diag_gemm_f32.py router"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "3m-asr-inference_amd"))
import numpy as np, torch
from m3asr import ops, _lib
from m3asr.plan import pack_wfrag


def report(title, n_groups=None):
    lib = _lib.load()
    buf = np.zeros(2048 * 8, dtype=np.uint64)
    lib.m3_debug_gemm_read.argtypes = [C.c_void_p, C.c_size_t]
    assert lib.m3_debug_gemm_read(buf.ctypes.data, buf.nbytes) == 0
    raw = buf.reshape(2048, 8)
    raw = raw[raw[:, 0] > 0] if n_groups is None else raw[:n_groups]   # (a smaller launch leaves the entries of earlier ones behind it)
    hw = ((raw[:, 7] >> np.uint64(40)) & np.uint64(0xffff)).astype(np.int64)
    xcc = ((raw[:, 7] >> np.uint64(56)) & np.uint64(0xf)).astype(np.int64)
    cu = (xcc << 16) | (hw & 0xff00)          # xcc | se_id[15:13] sh_id[12] cu_id[11:8]
    per_cu = np.bincount(np.unique(cu, return_inverse=True)[1])
    d = raw.astype(np.int64)
    d[:, 7] = (raw[:, 7] & np.uint64(0xffffffffff)).astype(np.int64)
    d[:, :7] = d[:, :7] & 0xffffffffff
    names = ["set-up", "load issue", "load wait", "MFMAs", "reduce+barrier", "epilogue", "store drain"]
    print("%s: %d work-groups" % (title, len(d)))
    for i, n in enumerate(names):
        v = d[:, i + 1] - d[:, i]
        print("  %-15s median %6d  (min %6d, max %6d)" % (n, np.median(v), v.min(), v.max()))
    print("  %-15s median %6d; first start -> last end %d cycles" % ("whole block", np.median(d[:, 7] - d[:, 0]), d[:, 7].max() - d[:, 0].min()))
    print("  placement: %d work-groups on %d distinct CUs; work-groups per CU: max %d, histogram %s" % (len(d), len(per_cu), per_cu.max(), np.bincount(per_cu)[1:].tolist()))


if sys.argv[1] == "router":
    from m3asr.config import EncoderConfig
    from m3asr.engine import Engine
    from m3asr.weights import make_weights
    cfg = EncoderConfig(output_dim=16, attention_dim=512, attention_heads=8, num_blocks=2, embed_heads=8, embed_dim=512, embed_linear_units=256,
                        embed_blocks=1, num_experts=32, hidden_units=256)
    eng = Engine.from_state_dict(cfg, make_weights(cfg, seed=5))
    eng.bind(torch.randn(1, 206, cfg.input_dim).cuda(), torch.tensor([[206]], dtype=torch.int32).cuda())
    at = eng.stage_names().index("blocks.0.moe_router")
    S = eng.buffer("x").numel() // cfg.attention_dim
    for _ in range(3):
        eng.run_stages(0, at + 1)
    torch.cuda.synchronize()
    report("router (acc_init, ln_out) M=%d N=%d K=%d" % (S, cfg.num_experts, 2 * cfg.attention_dim), n_groups=-(-S // 16) * -(-cfg.num_experts // 16))
    sys.exit(0)

M, N, K = (int(v) for v in sys.argv[1:4])
ln, cold = "ln" in sys.argv, "cold" in sys.argv
nw = 96 if cold else 1
a = torch.randn(M, K, device="cuda")
ws = [torch.randn(N, K, device="cuda") * K ** -0.5 for _ in range(nw)]
b = torch.randn(N, device="cuda")
wsum = torch.randn(N, device="cuda")
wbeta = torch.randn(N, device="cuda")
mask = "mask_out" if "mask_out" in sys.argv else ("mask_in" if "mask_in" in sys.argv else None)
lens = torch.tensor([max(M - 13, 0)], dtype=torch.int32, device="cuda")
y = torch.empty(M, N, device="cuda")
for frag in ([False, True] if "both" in sys.argv else ["frag" in sys.argv]):
    wl = [pack_wfrag(w) for w in ws] if frag else ws
    for i in range(max(3, nw)):
        ops.linear(a, wl[i % nw], b, out=y, ln_folded=(wsum, wbeta if mask == "mask_in" else None, 1e-12) if ln else None,
                   lens=lens if mask else None, rows_per_batch=M if mask else 0, mask_in=mask == "mask_in", mask_out=mask == "mask_out")
    torch.cuda.synchronize()
    report("M=%d N=%d K=%d ln=%s cold=%s frag=%s mask=%s" % (M, N, K, ln, cold, frag, mask))
