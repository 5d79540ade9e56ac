"""Audio in: samples -> the log-Mel feature frames the encoder reads (m3_fbank* in include/m3asr.h, csrc/fbank.hip).

Kaldi compute-fbank-feats with the options of a served model: 16 kHz mono PCM, int16 or float32 in the int16
value range; frames of 400 samples every 160 (snip_edges); per frame mean removal, pre-emphasis 0.97, Povey window, 512-point
power spectrum, `num_mel_bins` mel triangles from 20 Hz to Nyquist, log(max(E, FLT_EPSILON)).  No dither, no energy column,
no CMVN (that stays folded into conv1).

    fb = Fbank(cfg.input_dim, "cuda:0")
    feat, feat_len = fb(pcm)                       # pcm (B, N) or (N,) -> (B, T, bins) float32, (B,) int32 on the device

`num_frames`, `fbank_tables` and `AudioWindowBuffer` are host-only and need no GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from .serve import next_window_valid

SAMPLE_RATE, FRAME_LENGTH, FRAME_SHIFT, LOW_FREQ = 16000, 400, 160, 20.0
MAX_MEL_BINS = 128


def num_frames(n):
    """Frames of n samples (snip_edges): frame k reads samples [160 k, 160 k + 400)."""
    n = int(n)
    return 0 if n < FRAME_LENGTH else 1 + (n - FRAME_LENGTH) // FRAME_SHIFT


def _tables_image(num_mel_bins):
    lib = _lib.load()
    nbytes = lib.m3_fbank_tables_bytes(int(num_mel_bins))
    if nbytes == 0:
        raise _lib.M3Error("m3_fbank_tables_bytes failed: " + _lib.last_error())
    image = np.zeros(nbytes, dtype=np.uint8)
    check(lib.m3_fbank_tables_host(int(num_mel_bins), float(SAMPLE_RATE), LOW_FREQ, SAMPLE_RATE / 2.0,
                                   image.ctypes.data_as(C.c_void_p)), "m3_fbank_tables_host")
    return image


def fbank_tables(num_mel_bins):
    """The kernel's tables as the library builds them (float64 on the host, rounded once to float32), without a GPU:
    dict(window (400,), mel (bins, 256) weight of FFT bin j in mel bin m, twiddle256 / twiddle512 (256,) complex64,
    log_floor, image = the raw table image (uint8) that is uploaded)."""
    image = _tables_image(num_mel_bins)
    f32, i32 = image.view(np.float32), image.view(np.int32)
    assert int(i32[0]) == int(num_mel_bins)
    pos = 4
    tw256, pos = f32[pos:pos + 512].reshape(256, 2), pos + 512
    tw512, pos = f32[pos:pos + 512].reshape(256, 2), pos + 512
    window, pos = f32[pos:pos + FRAME_LENGTH].copy(), pos + FRAME_LENGTH
    lo, n, off = (i32[pos + MAX_MEL_BINS * k: pos + MAX_MEL_BINS * (k + 1)] for k in range(3))
    w = f32[pos + 3 * MAX_MEL_BINS:]
    mel = np.zeros((int(num_mel_bins), 256), dtype=np.float32)
    for m in range(int(num_mel_bins)):
        mel[m, lo[m]:lo[m] + n[m]] = w[off[m]:off[m] + n[m]]
    return dict(window=window, mel=mel, twiddle256=tw256[:, 0] + 1j * tw256[:, 1], twiddle512=tw512[:, 0] + 1j * tw512[:, 1],
                log_floor=float(f32[1]), image=image)


class Fbank:
    """The front end on one device: owns the uploaded tables; every call is one kernel launch."""

    def __init__(self, num_mel_bins, device="cuda:0"):
        self.lib = _lib.load()
        self.bins = int(num_mel_bins)
        self.device = torch.device(device)
        nbytes = self.lib.m3_fbank_tables_bytes(self.bins)
        if nbytes == 0:
            raise _lib.M3Error("m3_fbank_tables_bytes failed: " + _lib.last_error())
        with torch.cuda.device(self.device):
            self.tables = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            st = torch.cuda.current_stream()
            check(self.lib.m3_fbank_tables_init(self.bins, float(SAMPLE_RATE), LOW_FREQ, SAMPLE_RATE / 2.0, self.tables.data_ptr(),
                                                C.c_void_p(st.cuda_stream)), "m3_fbank_tables_init")

    def _device_pcm(self, pcm):
        """pcm as a (B, ld) int16 / float32 device tensor the kernel can read with 16-byte loads, and its sample count N."""
        pcm = torch.as_tensor(pcm)
        if pcm.dim() == 1:
            pcm = pcm.unsqueeze(0)
        if pcm.dim() != 2:
            raise ValueError("Fbank: pcm must be (B, N) or (N,), got %s" % (tuple(pcm.shape),))
        if pcm.dtype != torch.int16:
            pcm = pcm.to(torch.float32)
        B, N = int(pcm.shape[0]), int(pcm.shape[1])
        per16 = 16 // pcm.element_size()
        if pcm.device == self.device and N % per16 == 0 and pcm.stride(1) == 1 and pcm.stride(0) % per16 == 0 and \
                pcm.stride(0) >= N and pcm.data_ptr() % 16 == 0:
            return pcm, N
        ld = max(-(-N // per16) * per16, per16)
        dev = torch.empty(B, ld, dtype=pcm.dtype, device=self.device)
        dev[:, :N].copy_(pcm, non_blocking=True)
        return dev, N

    def __call__(self, pcm, n_samples=None, out=None, out_len=None, stream=None):
        """pcm (B, N) or (N,), int16 or float32 in the int16 range, tensor or array on any device; n_samples (B,) real samples
        per row (default N).  out: destination (B, T, >= bins) float32 on the device, rows of stride out.stride(1) (e.g. an
        engine input buffer; default a new (B, num_frames(N), bins) tensor); out_len: (B,) / (1, B) int32 destination of the
        frame counts.  Frames behind a row's last are written as zeros.  stream: torch stream (default the current one).
        -> (out, out_len)"""
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            st = torch.cuda.current_stream()
            dev, N = self._device_pcm(pcm)
            B = int(dev.shape[0])
            if n_samples is None:
                n_dev = torch.full((B,), N, dtype=torch.int32, device=self.device)
            else:
                n_dev = torch.as_tensor(n_samples).reshape(-1).to(self.device, torch.int32, non_blocking=True).clamp(max=N)
                if n_dev.numel() != B:
                    raise ValueError("Fbank: n_samples has %d entries for %d rows" % (n_dev.numel(), B))
            if out is None:
                out = torch.empty(B, num_frames(N), self.bins, dtype=torch.float32, device=self.device)
            if out.dim() != 3 or out.shape[0] != B or out.shape[2] < self.bins or out.dtype != torch.float32 or \
                    out.device != self.device or out.stride(2) != 1 or (B > 1 and out.shape[1] > 0 and out.stride(0) != out.shape[1] * out.stride(1)):
                raise ValueError("Fbank: out must be a (B, T, >= %d) float32 device tensor with dense rows" % self.bins)
            T = int(out.shape[1])
            if out_len is None:
                out_len = torch.zeros(B, dtype=torch.int32, device=self.device)
            if out_len.numel() != B or out_len.dtype != torch.int32 or out_len.device != self.device or not out_len.is_contiguous():
                raise ValueError("Fbank: out_len must be a contiguous int32 device tensor of %d entries" % B)
            if T == 0 or B == 0:                   # fewer than 400 samples everywhere: no frame, no launch
                out_len.zero_()
                return out, out_len
            check(self.lib.m3_fbank(self.tables.data_ptr(), dev.data_ptr(), int(dev.dtype == torch.int16), int(dev.stride(0)),
                                    n_dev.data_ptr(), B, T, self.bins, out.data_ptr(), int(out.stride(1)), out_len.data_ptr(),
                                    C.c_void_p(st.cuda_stream)), "m3_fbank")
        return out, out_len


class AudioWindowBuffer:
    """Samples of one stream, pushed in arbitrary pieces, handed back as the sample windows of chunked decoding: the
    sample-domain twin of serve.WindowBuffer.  Window n starts at sample 160 * 4 c n and holds the (4 c + 2) * 160 + 400
    samples of feature frames [4 c n, 4 c n + 4 c + 3)."""

    def __init__(self, chunk, dtype=torch.int16):
        self.c = int(chunk)
        self.hop = FRAME_SHIFT * 4 * self.c
        self.window = (4 * self.c + 2) * FRAME_SHIFT + FRAME_LENGTH
        self.dtype = dtype
        self.buf = torch.zeros(0, dtype=dtype)        # samples from sample self.base on
        self.base = 0
        self.total = 0
        self.chunks = 0
        self.ended = False

    def push(self, pcm):
        """int16 samples, or float32 in the int16 value range (rounded to the nearest int16 when the buffer holds int16)."""
        if self.ended:
            raise ValueError("push after end")
        pcm = torch.as_tensor(pcm).reshape(-1).cpu()
        if pcm.dtype.is_floating_point and not self.dtype.is_floating_point:
            pcm = pcm.round().clamp(-32768, 32767)
        self.buf = torch.cat([self.buf, pcm.to(self.dtype)])
        self.total += int(pcm.shape[0])

    def end(self):
        self.ended = True

    def rebase(self):
        """Start over at the next window: from here on the buffer behaves like a fresh one that was pushed every sample
        from sample 160 * 4 c * chunks on (serve.WindowBuffer.rebase in samples).  `ended` stays."""
        start = self.hop * self.chunks
        self.buf = self.buf[min(max(start - self.base, 0), self.buf.shape[0]):]
        self.total = max(self.total - start, 0)
        self.base = 0
        self.chunks = 0

    def ready(self):
        """Real FRAMES of the next window if it can run now, else 0 (the rule of serve.next_window_valid on frame counts)."""
        return next_window_valid(num_frames(self.total), self.chunks, self.c, self.ended)

    def drained(self):
        """The stream has ended and no further window will run."""
        return self.ended and self.ready() == 0

    def take(self, out=None):
        """The next window as (samples (window,) zero filled behind the real ones, count of real samples); advances by one
        chunk.  num_frames(count) is what ready() returned."""
        if self.ready() == 0:
            raise ValueError("no window ready")
        start = self.hop * self.chunks - self.base
        real = min(self.total - self.hop * self.chunks, self.window)
        win = torch.zeros(self.window, dtype=self.dtype) if out is None else out
        win.zero_()
        win[:real] = self.buf[start:start + real]
        self.chunks += 1
        drop = self.hop * self.chunks - self.base       # samples left of the next window are never read again
        if drop > 0:
            self.buf = self.buf[min(drop, self.buf.shape[0]):]
            self.base += drop
        return win, real
