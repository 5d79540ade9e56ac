"""Phase stamps of the fp32 attention core at T' = 50 (diagnostic build: make -C 3m-asr-inference_amd EXTRA=-DM3_ATT_DIAG
OBJDIR=build_adiag LIB=../tools/_diag_att.so; run with M3ASR_LIB=tools/_diag_att.so).  Median shader-clock cycles of wave 0 over
the work-groups of the LAST launch, per phase:
  arguments (the kernel-argument loads) | operands (work-group id arithmetic, addresses, every load of Q and of the first key tile,
  and the wait for them) | scores (the K / P MFMA chain) | softmax | P.V (the transposed read of the probabilities and its
  MFMAs) | barrier (partial state to LDS, wait for the other three waves) | merge (factors, output elements, store drain).
The stamps fence the instruction stream, so the build is slower than the product: read the SHARES, not the length.
Shapes: dk = 64, H = 8 (the main encoder's blocks) and dk = 128, H = 4 (the embed encoder's), B = 1, full length.
usage: diag_attention.py [T]      (default 50)"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "3m-asr-inference_amd"))
import numpy as np, torch
from m3asr import ops, _lib

NAMES = ["arguments", "operands", "scores", "softmax", "P.V", "barrier", "merge"]


def report(title, n_groups):
    lib = _lib.load()
    buf = np.zeros(2048 * 8, dtype=np.uint64)
    lib.m3_debug_att_read.argtypes = [C.c_void_p, C.c_size_t]
    assert lib.m3_debug_att_read(buf.ctypes.data, buf.nbytes) == 0
    d = buf.reshape(2048, 8)[:n_groups].astype(np.int64)
    assert (d[:, 0] > 0).all(), "a work-group of the launch left no stamps"
    print("%s: %d work-groups" % (title, len(d)))
    for i, n in enumerate(NAMES):
        v = d[:, i + 1] - d[:, i]
        print("  %-10s median %6d  (min %6d, max %6d)" % (n, np.median(v), v.min(), v.max()))
    print("  %-10s median %6d" % ("whole wave", np.median(d[:, 7] - d[:, 0])))


T = int(sys.argv[1]) if len(sys.argv) > 1 else 50
for H, dk in ((8, 64), (4, 128)):
    D = H * dk
    g = torch.Generator().manual_seed(0)
    qkv, p = torch.randn(T, 3 * D, generator=g).cuda(), torch.randn(T, D, generator=g).cuda()
    u, v = (torch.randn(H, dk, generator=g) * 0.3).cuda(), (torch.randn(H, dk, generator=g) * 0.3).cuda()
    lens = torch.tensor([T], dtype=torch.int32).cuda()
    out = torch.empty(T, D, device="cuda")
    for _ in range(5):
        ops.relpos_attention(qkv, p, u, v, lens, 1, T, H, dk, out=out)
    torch.cuda.synchronize()
    report("dk=%d H=%d T'=%d" % (dk, H, T), -(-T // 16) * H)
