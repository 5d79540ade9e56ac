"""Audio in: samples -> the log-Mel feature frames the encoder reads (m3_fbank* in include/m3asr.h, csrc/fbank.hip).

Kaldi compute-fbank-feats with the options of a served model: 16 kHz mono PCM, int16 or float32 in the int16
value range; frames of 400 samples every 160 (snip_edges); per frame mean removal, pre-emphasis 0.97, Povey window, 512-point
power spectrum, `num_mel_bins` mel triangles from 20 Hz to Nyquist, log(max(E, FLT_EPSILON)).  No dither, no energy column,
no CMVN (that stays folded into conv1).

    fb = Fbank(cfg.input_dim, "cuda:0")
    feat, feat_len = fb(pcm)                       # pcm (B, N) or (N,) -> (B, T, bins) float32, (B,) int32 on the device

Delta features (m3_add_deltas, csrc/deltas.hip): a model trained on the loader's add_deltas reads
static | delta | delta-delta columns; DeltaFbank is Fbank followed by one more launch that fills them in.

    fb = DeltaFbank(cfg.num_mel_bins, cfg.delta_order, cfg.delta_window, "cuda:0")
    feat, feat_len = fb(pcm)                       # (B, T, (order + 1) * bins)

Long recordings (m3_vad_*, m3_segment_gather, csrc/vad.hip): EnergyVad is Kaldi's compute-vad on frame
log-energy plus a segmenter, three launches; segment_gather cuts feature rows into an engine batch (m3asr.longform drives both).

    segs = EnergyVad(VadConfig(), "cuda:0")(pcm)   # [(start, end)] in frames per row

`num_frames`, `fbank_tables`, `delta_tables`, `VadConfig` and `AudioWindowBuffer` are host-only and need no GPU.
"""
import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib
from ._lib import check
from .serve import next_window_valid

SAMPLE_RATE, FRAME_LENGTH, FRAME_SHIFT, LOW_FREQ = 16000, 400, 160, 20.0
MAX_MEL_BINS = 128
MAX_DELTA_CONTEXT = 8


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


def delta_context(order, window):
    """Frames of context on either side that a delta frame reads: order * window (0 for order 0)."""
    return int(order) * int(window)


def delta_tables(order, window):
    """Kaldi's DeltaFeatures filters as the library builds them (float64 on the host, rounded once to float32), without a
    GPU: [scales_0, ..., scales_order], scales_i a float32 array of 2 i window + 1 taps for offsets -i window .. i window."""
    rows = np.zeros((int(order) + 1, 2 * MAX_DELTA_CONTEXT + 1), dtype=np.float32)
    check(_lib.load().m3_deltas_tables_host(int(order), int(window), rows.ctypes.data_as(C.c_void_p)), "m3_deltas_tables_host")
    return [rows[i, MAX_DELTA_CONTEXT - i * int(window): MAX_DELTA_CONTEXT + i * int(window) + 1].copy() for i in range(int(order) + 1)]


def add_deltas(feat, n_in, order, window, out=None, lead=None, n_out=None, out_len=None, bins=None, stream=None):
    """m3_add_deltas on device tensors: feat (B, T_in, >= bins) float32 static frames (bins: default feat.shape[2]), n_in (B,)
    int32 frames present; lead (B,) int32 frames in front that are context only (None = 0), n_out (B,) int32 frames to
    produce (None = n_in).  out (B, T_out, >= (order + 1) * bins) (default a new dense (B, T_in, (order + 1) * bins) tensor);
    out is feat: the in-place form, only the delta columns are written.  out_len (B,) int32 receives the clipped n_out.
    -> out"""
    lib = _lib.load()
    bins = int(feat.shape[2] if bins is None else bins)
    B = int(feat.shape[0])
    width = (int(order) + 1) * bins
    if feat.dim() != 3 or feat.dtype != torch.float32 or not feat.is_cuda or (feat.shape[2] > 1 and feat.stride(2) != 1) or feat.shape[2] < bins:
        raise ValueError("add_deltas: feat must be a (B, T, >= %d) float32 device tensor with dense rows" % bins)
    if out is None:
        out = torch.empty(B, int(feat.shape[1]), width, dtype=torch.float32, device=feat.device)
    if out.dim() != 3 or out.shape[0] != B or out.shape[2] < width or out.dtype != torch.float32 or out.device != feat.device or \
            out.stride(2) != 1:
        raise ValueError("add_deltas: out must be a (B, T, >= %d) float32 device tensor with dense rows" % width)
    n_out = n_in if n_out is None else n_out
    for name, v in (("n_in", n_in), ("lead", lead), ("n_out", n_out), ("out_len", out_len)):
        if v is None and name in ("lead", "out_len"):
            continue
        if v.dtype != torch.int32 or v.device != feat.device or v.numel() != B or not v.is_contiguous():
            raise ValueError("add_deltas: %s must be a contiguous int32 device tensor of %d entries" % (name, B))
    ptr = lambda v: None if v is None else v.data_ptr()
    with torch.cuda.device(feat.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        st = torch.cuda.current_stream()
        check(lib.m3_add_deltas(feat.data_ptr(), int(feat.stride(1)), int(feat.stride(0)), int(feat.shape[1]), n_in.data_ptr(),
                                ptr(lead), n_out.data_ptr(), B, int(out.shape[1]), bins, int(order), int(window),
                                out.data_ptr(), int(out.stride(1)), int(out.stride(0)), ptr(out_len), C.c_void_p(st.cuda_stream)),
              "m3_add_deltas")
    return out


class DeltaFbank:
    """Fbank followed by Kaldi's add-deltas on one device: what the loader's add_deltas / delta_window feed a
    model.  It has Fbank's call signature and makes two launches: the log-Mel frames go into columns [0, bins) of `out`, whose
    rows are (order + 1) * bins wide or wider, then m3_add_deltas in its in-place form fills in the delta blocks beside them."""

    def __init__(self, num_mel_bins, order=2, window=2, device="cuda:0"):
        self.order, self.delta_window = int(order), int(window)
        delta_tables(self.order, self.delta_window)              # refuses a bad (order, window) here, with the library's message
        self.fbank = Fbank(num_mel_bins, device)
        self.bins, self.device, self.lib = self.fbank.bins, self.fbank.device, self.fbank.lib
        self.width = (self.order + 1) * self.bins
        self.context = delta_context(self.order, self.delta_window)

    def __call__(self, pcm, n_samples=None, out=None, out_len=None, stream=None, lead=None, n_out=None):
        """Fbank.__call__ with rows of (order + 1) * bins columns: out (B, T, >= width), default a new (B, num_frames(N), width)
        tensor.  lead / n_out (B,) int32, host or device (the streaming form): the samples are a window whose first lead[b]
        frames are context only and of which n_out[b] delta frames are wanted; the static frames then go through a scratch
        tensor and out may have fewer rows than the window has frames.  Without them every frame is produced, with Kaldi's edge
        replication at both ends.  -> (out, out_len)"""
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            st = torch.cuda.current_stream()
            if lead is None and n_out is None:
                if out is None:
                    pcm = torch.as_tensor(pcm)
                    shape = (1, pcm.shape[0]) if pcm.dim() == 1 else tuple(pcm.shape)
                    out = torch.empty(int(shape[0]), num_frames(shape[1]), self.width, dtype=torch.float32, device=self.device)
                if out.dim() != 3 or out.shape[2] < self.width:
                    raise ValueError("DeltaFbank: out must be a (B, T, >= %d) float32 device tensor with dense rows" % self.width)
                out, out_len = self.fbank(pcm, n_samples, out=out, out_len=out_len, stream=st)
                if out.shape[0] and out.shape[1]:
                    add_deltas(out, out_len.view(-1), self.order, self.delta_window, out=out, bins=self.bins, stream=st)
                return out, out_len
            if lead is None or n_out is None or out is None:
                raise ValueError("DeltaFbank: the streaming form needs lead, n_out and out")
            dev, N = self.fbank._device_pcm(pcm)
            B, T_in = int(dev.shape[0]), max(num_frames(N), 1)
            key = (B, T_in)
            if getattr(self, "_scratch_key", None) != key:
                self._scratch = torch.empty(B, T_in, -(-self.bins // 4) * 4, dtype=torch.float32, device=self.device)
                self._scratch_len = torch.zeros(B, dtype=torch.int32, device=self.device)
                self._scratch_key = key
            lead = torch.as_tensor(lead).reshape(-1).to(self.device, torch.int32, non_blocking=True)
            n_out = torch.as_tensor(n_out).reshape(-1).to(self.device, torch.int32, non_blocking=True)
            if out_len is None:
                out_len = torch.zeros(B, dtype=torch.int32, device=self.device)
            if num_frames(N) == 0 or B == 0:
                out[..., :self.width].zero_()
                out_len.zero_()
                return out, out_len
            self.fbank(dev, n_samples, out=self._scratch, out_len=self._scratch_len, stream=st)
            add_deltas(self._scratch, self._scratch_len, self.order, self.delta_window, out=out, lead=lead, n_out=n_out,
                       out_len=out_len.view(-1), bins=self.bins, stream=st)
        return out, out_len


def make_frontend(cfg, device):
    """The front end a config's encoder reads: Fbank(cfg.input_dim), or DeltaFbank when the model was trained on delta features
    (cfg.delta_order > 0)."""
    if cfg.delta_order > 0:
        return DeltaFbank(cfg.num_mel_bins, cfg.delta_order, cfg.delta_window, device)
    return Fbank(cfg.input_dim, device)


def _checked_context(context):
    context = int(context)
    if not 0 <= context <= MAX_DELTA_CONTEXT:
        raise ValueError("AudioWindowBuffer: context=%d outside [0, %d]" % (context, MAX_DELTA_CONTEXT))
    return context


def _context_window(frames, n, c, v, R):
    """The static frames [s0, s1) that window n of v delta frames reads out of `frames` there are, and its lead (DESIGN.md
    32.5): R frames of context on either side where the segment has them."""
    s0 = max(4 * c * n - R, 0)
    s1 = min(4 * c * n + v + R, frames)
    return s0, s1, 4 * c * n - s0


def _check_rates(rate_in, rate_out):
    lib = _lib.load()
    if lib.m3_resample_tables_bytes(int(rate_in), int(rate_out)) == 0:
        raise _lib.M3Error("m3_resample_tables_bytes failed: " + _lib.last_error())
    return lib


def num_resampled(n, rate_in, rate_out=SAMPLE_RATE, flush=True):
    """Samples at rate_out that n samples at rate_in give (m3_resample_num_samples).  flush=False: those that can be computed
    now, while more input may come -- none of them reads a sample at or beyond n; flush=True: the stream has ended."""
    got = _lib.load().m3_resample_num_samples(int(rate_in), int(rate_out), int(n), int(bool(flush)))
    if got < 0:
        raise _lib.M3Error("m3_resample_num_samples failed: " + _lib.last_error())
    return int(got)


def resample_span(out0, n_out, rate_in, rate_out=SAMPLE_RATE):
    """[first_in, end_in): the absolute input samples that outputs [out0, out0 + n_out) read; first_in may be negative."""
    f, e = C.c_int64(0), C.c_int64(0)
    check(_lib.load().m3_resample_input_span(int(rate_in), int(rate_out), int(out0), int(n_out), C.byref(f), C.byref(e)),
          "m3_resample_input_span")
    return int(f.value), int(e.value)


def resample_tables(rate_in, rate_out=SAMPLE_RATE):
    """The resampler's tables as the library builds them (float64 on the host, every weight rounded once to float32), without
    a GPU: dict(first (phases,) int32, n (phases,) int32, weights (phases, max_taps) float32 with zeros behind n[p], in_unit,
    out_unit, image = the raw table image (uint8) that is uploaded)."""
    lib = _check_rates(rate_in, rate_out)
    image = np.zeros(lib.m3_resample_tables_bytes(int(rate_in), int(rate_out)), dtype=np.uint8)
    check(lib.m3_resample_tables_host(int(rate_in), int(rate_out), image.ctypes.data_as(C.c_void_p)), "m3_resample_tables_host")
    i32, f32 = image.view(np.int32), image.view(np.float32)
    assert (int(i32[0]), int(i32[1])) == (int(rate_in), int(rate_out))
    in_unit, out_unit, max_taps, w_off = (int(v) for v in i32[2:6])
    first, n = i32[8:8 + out_unit].copy(), i32[8 + out_unit:8 + 2 * out_unit].copy()
    weights = f32[w_off:w_off + max_taps * out_unit].reshape(max_taps, out_unit).T.copy()
    return dict(first=first, n=n, weights=weights, in_unit=in_unit, out_unit=out_unit, image=image)


class Resampler:
    """Kaldi's LinearResample on one device (m3_resample* in include/m3asr.h): owns the uploaded table of one
    rate pair; every call is one kernel launch.  channels: interleaved channels per sample of the input; channel: -1 = the
    mean of all channels, k = channel k alone."""

    def __init__(self, rate_in, device="cuda:0", rate_out=SAMPLE_RATE, channels=1, channel=-1):
        self.lib = _check_rates(rate_in, rate_out)
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.channels, self.channel = int(channels), int(channel)
        if not 1 <= self.channels <= 8:
            raise ValueError("Resampler: channels=%d outside [1, 8]" % self.channels)
        if not -1 <= self.channel < self.channels:
            raise ValueError("Resampler: channel=%d outside [-1, %d)" % (self.channel, self.channels))
        self.device = torch.device(device)
        g = int(np.gcd(self.rate_in, self.rate_out))
        self.in_unit, self.out_unit = self.rate_in // g, self.rate_out // g
        nbytes = self.lib.m3_resample_tables_bytes(self.rate_in, self.rate_out)
        with torch.cuda.device(self.device):
            self.tables = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            st = torch.cuda.current_stream()
            check(self.lib.m3_resample_tables_init(self.rate_in, self.rate_out, self.tables.data_ptr(), C.c_void_p(st.cuda_stream)),
                  "m3_resample_tables_init")

    def num_samples(self, n, flush=True):
        return num_resampled(n, self.rate_in, self.rate_out, flush)

    def _device_pcm(self, pcm):
        """pcm as a (B, ld) int16 / float32 device tensor of interleaved channels that the kernel can read with 16-byte loads,
        and its samples per channel N (the staging rule of Fbank._device_pcm)."""
        pcm = torch.as_tensor(pcm)
        if pcm.dim() == 1:
            pcm = pcm.unsqueeze(0)
        if pcm.dim() == 3:
            if pcm.shape[2] != self.channels:
                raise ValueError("Resampler: pcm has %d channels, the resampler was built for %d" % (pcm.shape[2], self.channels))
            if pcm.stride(2) != 1 or pcm.stride(1) != self.channels:
                pcm = pcm.contiguous()
            pcm = pcm.as_strided((pcm.shape[0], pcm.shape[1] * self.channels), (pcm.stride(0), 1))
        if pcm.dim() != 2 or pcm.shape[1] % self.channels:
            raise ValueError("Resampler: pcm must be (B, N * %d), (B, N, %d) or (N,), got %s" % (
                self.channels, self.channels, tuple(pcm.shape)))
        if pcm.dtype != torch.int16:
            pcm = pcm.to(torch.float32)
        B, W = int(pcm.shape[0]), int(pcm.shape[1])
        per16 = 16 // pcm.element_size()
        if pcm.device == self.device and W % per16 == 0 and pcm.stride(1) == 1 and pcm.stride(0) % per16 == 0 and \
                pcm.stride(0) >= W and pcm.data_ptr() % 16 == 0:
            return pcm, W // self.channels
        ld = max(-(-W // per16) * per16, per16)
        dev = torch.empty(B, ld, dtype=pcm.dtype, device=self.device)
        dev[:, :W].copy_(pcm, non_blocking=True)
        return dev, W // self.channels

    def launch(self, pcm, in0, n_in, out0, n_out, out, stream=None):
        """The launch itself, for the streaming path: pcm (B, ld) int16 / float32 DEVICE tensor of interleaved channels (16-byte
        aligned rows), in0 / out0 (B,) int64 and n_in / n_out (B,) int32 device vectors (the m3_resample block of
        include/m3asr.h), out (B, N_out) float32 device tensor with unit column stride.  -> out"""
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            st = torch.cuda.current_stream()
            B = int(pcm.shape[0])
            if pcm.dim() != 2 or pcm.device != self.device or pcm.dtype not in (torch.int16, torch.float32) or pcm.stride(1) != 1:
                raise ValueError("Resampler.launch: pcm must be a (B, ld) int16 / float32 device tensor with dense rows")
            if out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or out.device != self.device or out.stride(1) != 1:
                raise ValueError("Resampler.launch: out must be a (B, N_out) float32 device tensor with dense rows")
            for name, v, dt in (("in0", in0, torch.int64), ("n_in", n_in, torch.int32), ("out0", out0, torch.int64),
                                ("n_out", n_out, torch.int32)):
                if v.dtype != dt or v.device != self.device or v.numel() != B or not v.is_contiguous():
                    raise ValueError("Resampler.launch: %s must be a contiguous %s device tensor of %d entries" % (name, dt, B))
            if B == 0 or out.shape[1] == 0:
                return out
            check(self.lib.m3_resample(self.tables.data_ptr(), pcm.data_ptr(), int(pcm.dtype == torch.int16), self.channels,
                                       self.channel, int(pcm.stride(0)), in0.data_ptr(), n_in.data_ptr(), out0.data_ptr(),
                                       n_out.data_ptr(), B, int(out.shape[1]), out.data_ptr(), int(out.stride(0)),
                                       C.c_void_p(st.cuda_stream)), "m3_resample")
        return out

    def __call__(self, pcm, n_samples=None, out=None, stream=None):
        """The offline resample, one launch: pcm (B, N), (N,) or (B, N, channels) (interleaved: (B, N * channels)), int16 or
        float32, tensor or array on any device; n_samples (B,) real samples per channel and row (default N).  The signal is
        flushed: its future is zeros.  out: destination (B, N_out) float32 on the device (default a new
        (B, num_samples(N)) tensor); columns behind a row's count are written as zeros.
        -> (out, n_out (B,) int32 on the device)"""
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            dev, N = self._device_pcm(pcm)
            B = int(dev.shape[0])
            if n_samples is None:
                n_in = torch.full((B,), N, dtype=torch.int32, device=self.device)
            else:
                n_in = torch.as_tensor(n_samples).reshape(-1).to(self.device, torch.int32, non_blocking=True).clamp(min=0, max=N)
                if n_in.numel() != B:
                    raise ValueError("Resampler: n_samples has %d entries for %d rows" % (n_in.numel(), B))
            if out is None:
                out = torch.empty(B, self.num_samples(N), dtype=torch.float32, device=self.device)
            if self.rate_in == self.rate_out:
                n_out = n_in.clone()
            else:                                      # the flushed count: ceil(n * out_unit / in_unit)
                n_out = ((n_in.to(torch.int64) * self.out_unit + (self.in_unit - 1)) // self.in_unit).to(torch.int32)
            n_out = n_out.clamp(max=int(out.shape[1])) if out.dim() == 2 else n_out
            zero = torch.zeros(B, dtype=torch.int64, device=self.device)
            self.launch(dev, zero, n_in, zero, n_out, out, stream=torch.cuda.current_stream())
        return out, n_out


class ResampledWindowBuffer:
    """AudioWindowBuffer for a stream at another rate or with several channels: what AudioWindowBuffer(chunk, dtype,
    sample_rate, channels) returns unless both have their defaults.  It buffers INPUT-rate interleaved samples and keeps
    absolute clocks: the 16 kHz signal is resample(whole session) (m3_resample's contract makes a sample depend on its
    absolute index only), window n of the open segment holds its samples [origin + hop n, origin + hop n + window), and take()
    hands back the input samples that window reads together with the four index entries of its row of the launch.
    context=R: as in AudioWindowBuffer, in 16 kHz frames of the open segment."""

    def __init__(self, chunk, dtype=torch.int16, sample_rate=SAMPLE_RATE, channels=1, context=0):
        self.c = int(chunk)
        self.context = _checked_context(context)
        self.lead = 0
        self.hop = FRAME_SHIFT * 4 * self.c
        self.window = (4 * self.c + 2 + 2 * self.context) * FRAME_SHIFT + FRAME_LENGTH
        self.dtype = dtype
        self.rate, self.channels = int(sample_rate), int(channels)
        _check_rates(self.rate, SAMPLE_RATE)
        if not 1 <= self.channels <= 8:
            raise ValueError("AudioWindowBuffer: channels=%d outside [1, 8]" % self.channels)
        lo, hi = resample_span(0, self.window, self.rate)
        self.span = hi - lo + 1                        # input samples a window reads, at any phase of its first output
        self.buf = torch.zeros(0, self.channels, dtype=dtype)   # input samples from absolute input sample self.base on
        self.base = 0
        self.total = 0                                 # input samples per channel received since the session began
        self.origin = 0                                # absolute 16 kHz sample at which the open segment starts
        self.chunks = 0
        self.ended = False

    def push(self, pcm):
        """(n, channels) or interleaved (n * channels,) samples at the input rate: int16, or float32 in the int16 value range
        (rounded to the nearest int16 when the buffer holds int16)."""
        if self.ended:
            raise ValueError("push after end")
        pcm = torch.as_tensor(pcm).cpu()
        if pcm.numel() % self.channels:
            raise ValueError("push: %d values are no whole samples of %d channels" % (pcm.numel(), self.channels))
        pcm = pcm.reshape(-1, self.channels)
        if pcm.dtype.is_floating_point and not self.dtype.is_floating_point:
            pcm = pcm.round().clamp(-32768, 32767)
        self.buf = torch.cat([self.buf, pcm.to(self.dtype)])
        self.total += int(pcm.shape[0])

    def end(self):
        self.ended = True

    def rebase(self):
        """Start the next segment at the next window.  Only the 16 kHz origin moves: the sample clocks run on and nothing is
        zeroed at the cut, so the next segment's samples are exactly resample(whole session)[origin:].  `ended` stays."""
        self.origin += self.hop * self.chunks
        self.chunks = 0

    def _available(self):
        """16 kHz samples of the open segment that can be computed now"""
        return max(num_resampled(self.total, self.rate, SAMPLE_RATE, flush=self.ended) - self.origin, 0)

    def ready(self):
        """Real FRAMES of the next window if it can run now, else 0 (serve.next_window_valid on the frames of the resampled
        samples there are)."""
        frames = num_frames(self._available())
        return next_window_valid(frames if self.ended else max(frames - self.context, 0), self.chunks, self.c, self.ended)

    def drained(self):
        return self.ended and self.ready() == 0

    def take(self, out=None):
        """The next window as (input samples (span, channels) zero filled behind the real ones, in0, n_in, out0, n_out): the
        row's entries of the resampler launch that produces the window's n_out real 16 kHz samples; advances by one chunk.
        num_frames(n_out) is what ready() returned -- with context > 0, that plus the frames of context in front (self.lead
        after the call) and behind.  out: a (span * channels,) or (span, channels) destination."""
        v = self.ready()
        if v == 0:
            raise ValueError("no window ready")
        avail = self._available()
        s0, s1, self.lead = _context_window(num_frames(avail), self.chunks, self.c, v, self.context)
        out0 = self.origin + FRAME_SHIFT * s0
        n_out = min(avail - FRAME_SHIFT * s0 if s1 == num_frames(avail) else FRAME_SHIFT * (s1 - s0 - 1) + FRAME_LENGTH, self.window)
        lo, hi = resample_span(out0, n_out, self.rate)
        in0, end = max(lo, self.base), min(hi, self.total)
        n_in = max(end - in0, 0)
        win = torch.zeros(self.span, self.channels, dtype=self.dtype) if out is None else out
        win.zero_()
        win.view(-1, self.channels)[:n_in] = self.buf[in0 - self.base:in0 - self.base + n_in]
        self.chunks += 1
        keep = self.origin + FRAME_SHIFT * max(4 * self.c * self.chunks - self.context, 0)
        drop = resample_span(keep, 1, self.rate)[0] - self.base   # input left of the next window is never read again
        if drop > 0:
            self.buf = self.buf[min(drop, self.buf.shape[0]):]
            self.base += drop
        return win, in0, n_in, out0, n_out


class AudioWindowBuffer:
    """Samples of one stream, pushed in arbitrary pieces, handed back as the sample windows of chunked decoding: the
    sample-domain twin of serve.WindowBuffer.  Window n starts at sample 160 * 4 c n and holds the (4 c + 2) * 160 + 400
    samples of feature frames [4 c n, 4 c n + 4 c + 3).  With another sample_rate or channels > 1 the constructor hands out
    a ResampledWindowBuffer instead, which keeps the input-rate samples.

    context=R > 0, for a front end with delta features (DeltaFbank, R = order * window): a delta frame exists once its R frames
    of lookahead do, or the stream has ended, so ready() counts F - R of the F frames there are until then.  take() hands back
    the samples of static frames [s0, s1), s0 = max(4 c n - R, 0), s1 = min(4 c n + v + R, F), and leaves in self.lead the
    4 c n - s0 frames in front that are context only: 0 for the first window of a segment, R later (fewer while 4 c n < R).
    The window then holds up to (4 c + 2 + 2 R) * 160 + 400 samples, and the buffer keeps its samples from frame
    max(4 c (n + 1) - R, 0) on.  After rebase() the segment is a fresh stream: no context in front of the cut."""

    def __new__(cls, chunk, dtype=torch.int16, sample_rate=SAMPLE_RATE, channels=1, context=0):
        if cls is AudioWindowBuffer and (int(sample_rate) != SAMPLE_RATE or int(channels) != 1):
            return ResampledWindowBuffer(chunk, dtype, sample_rate, channels, context)
        return super().__new__(cls)

    context = 0       # frames of context on either side (an instance field only where it is not 0: the plain buffer keeps its fields)
    lead = 0          # frames of context in front of the window take() handed out last

    def __init__(self, chunk, dtype=torch.int16, sample_rate=SAMPLE_RATE, channels=1, context=0):
        self.c = int(chunk)
        if _checked_context(context):
            self.context = int(context)
        self.hop = FRAME_SHIFT * 4 * self.c
        self.window = (4 * self.c + 2 + 2 * self.context) * FRAME_SHIFT + FRAME_LENGTH
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
        frames = num_frames(self.total)
        return next_window_valid(frames if self.ended else max(frames - self.context, 0), self.chunks, self.c, self.ended)

    def drained(self):
        """The stream has ended and no further window will run."""
        return self.ended and self.ready() == 0

    def take(self, out=None):
        """The next window as (samples (window,) zero filled behind the real ones, count of real samples); advances by one
        chunk.  num_frames(count) is what ready() returned -- with context > 0, that plus the frames of context in front
        (self.lead after the call) and behind."""
        v = self.ready()
        if v == 0:
            raise ValueError("no window ready")
        frames = num_frames(self.total)
        s0, s1, self.lead = _context_window(frames, self.chunks, self.c, v, self.context)
        start = FRAME_SHIFT * s0 - self.base
        real = min(self.total - FRAME_SHIFT * s0 if s1 == frames else FRAME_SHIFT * (s1 - s0 - 1) + FRAME_LENGTH, self.window)
        win = torch.zeros(self.window, dtype=self.dtype) if out is None else out
        win.zero_()
        win[:real] = self.buf[start:start + real]
        self.chunks += 1
        drop = FRAME_SHIFT * max(4 * self.c * self.chunks - self.context, 0) - self.base   # samples left of the next window are never read again
        if drop > 0:
            self.buf = self.buf[min(drop, self.buf.shape[0]):]
            self.base += drop
        return win, real


MAX_VAD_CONTEXT = 32
FRAME_MS = 1000 * FRAME_SHIFT // SAMPLE_RATE


@dataclasses.dataclass
class VadConfig:
    """Energy VAD and segmenter options (m3_vad_* in include/m3asr.h).  The first four are Kaldi's compute-vad
    options with Kaldi's defaults; the segmenter's are in 10-ms feature frames (`frames(ms)` converts) and nobody has tuned
    them: min_silence = a pause shorter than this does not cut, min_speech = a voiced run shorter than this is dropped, pad =
    frames kept on either side of a run, max_segment = the longest segment, split_search = how far back from max_segment the
    quietest frame is looked for when a run has to be cut.  Refused: context outside [0, 32], proportion_threshold outside
    (0, 1), a negative energy_mean_scale, min_silence or pad, min_speech < 7, 2 pad > min_silence, split_search outside
    [1, max_segment - 7]."""
    energy_threshold: float = 5.0
    energy_mean_scale: float = 0.5
    context: int = 0
    proportion_threshold: float = 0.6
    min_silence: int = 30
    min_speech: int = 20
    pad: int = 10
    max_segment: int = 3000
    split_search: int = 500
    frame_ms: int = FRAME_MS

    def __post_init__(self):
        self.energy_threshold, self.energy_mean_scale = float(self.energy_threshold), float(self.energy_mean_scale)
        self.context, self.proportion_threshold = int(self.context), float(self.proportion_threshold)
        self.min_silence, self.min_speech, self.pad = int(self.min_silence), int(self.min_speech), int(self.pad)
        self.max_segment, self.split_search = int(self.max_segment), int(self.split_search)
        if self.energy_threshold != self.energy_threshold:
            raise ValueError("VadConfig: energy_threshold is not a number")
        if not 0 <= self.context <= MAX_VAD_CONTEXT:
            raise ValueError("VadConfig: context=%d outside [0, %d]" % (self.context, MAX_VAD_CONTEXT))
        if not 0.0 < self.proportion_threshold < 1.0:
            raise ValueError("VadConfig: proportion_threshold=%g outside (0, 1)" % self.proportion_threshold)
        if not 0.0 <= self.energy_mean_scale < float("inf"):
            raise ValueError("VadConfig: energy_mean_scale=%g is negative or not finite" % self.energy_mean_scale)
        if self.min_silence < 0 or self.pad < 0:
            raise ValueError("VadConfig: min_silence=%d or pad=%d is negative" % (self.min_silence, self.pad))
        if self.min_speech < 7:
            raise ValueError("VadConfig: min_speech=%d is below 7 frames (the encoder's shortest input)" % self.min_speech)
        if 2 * self.pad > self.min_silence:
            raise ValueError("VadConfig: 2 * pad=%d exceeds min_silence=%d (padded runs could touch)" % (2 * self.pad, self.min_silence))
        if not 1 <= self.split_search <= self.max_segment - 7:
            raise ValueError("VadConfig: split_search=%d outside [1, max_segment - 7 = %d]" % (self.split_search, self.max_segment - 7))

    def frames(self, ms):
        """ceil(ms / frame_ms)"""
        return int(-(-ms // self.frame_ms)) if isinstance(ms, int) else int(np.ceil(ms / self.frame_ms))

    def segment_options(self):
        return self.min_silence, self.min_speech, self.pad, self.max_segment, self.split_search


class EnergyVad:
    """Kaldi's energy VAD and the segmenter on one device (m3_vad_* in include/m3asr.h, csrc/vad.hip).
    log_energy, decide and segments each wrap one launch; __call__ runs the three and brings the segment lists to the host."""

    def __init__(self, cfg=None, device="cuda:0"):
        self.cfg = VadConfig() if cfg is None else cfg
        self.lib = _lib.load()
        self.device = torch.device(device)

    def _on(self, stream):
        return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())

    def _lens(self, name, v, B):
        if v.dtype != torch.int32 or v.device != self.device or v.numel() != B or not v.is_contiguous():
            raise ValueError("EnergyVad: %s must be a contiguous int32 device tensor of %d entries" % (name, B))
        return v.view(-1)

    def _matrix(self, name, m, dtype, B=None):
        if m.dim() != 2 or m.dtype != dtype or m.device != self.device or (m.shape[1] > 1 and m.stride(1) != 1) or \
                (B is not None and m.shape[0] != B):
            raise ValueError("EnergyVad: %s must be a (B, T) %s device tensor with dense rows" % (name, dtype))
        return m

    def log_energy(self, pcm, n_samples=None, out=None, out_len=None, stream=None):
        """pcm (B, N) or (N,), int16 or float32 in the int16 range, on any device; n_samples (B,) real samples per row.
        -> (logE (B, T = num_frames(N)) float32, lens (B,) int32) on the device; frames behind a row's last are zeros."""
        with torch.cuda.device(self.device), self._on(stream):
            st = torch.cuda.current_stream()
            dev, N = Fbank._device_pcm(self, pcm)           # the staging rule of the feature front end
            B = int(dev.shape[0])
            if n_samples is None:
                n_dev = torch.full((B,), N, dtype=torch.int32, device=self.device)
            else:
                n_dev = torch.as_tensor(n_samples).reshape(-1).to(self.device, torch.int32, non_blocking=True).clamp(max=N)
                if n_dev.numel() != B:
                    raise ValueError("EnergyVad: n_samples has %d entries for %d rows" % (n_dev.numel(), B))
            if out is None:
                out = torch.empty(B, num_frames(N), dtype=torch.float32, device=self.device)
            self._matrix("out", out, torch.float32, B)
            if out_len is None:
                out_len = torch.zeros(B, dtype=torch.int32, device=self.device)
            self._lens("out_len", out_len, B)
            T = int(out.shape[1])
            if B == 0 or T == 0:
                out_len.zero_()
                return out, out_len
            check(self.lib.m3_vad_log_energy(dev.data_ptr(), int(dev.dtype == torch.int16), int(dev.stride(0)), n_dev.data_ptr(), B, T,
                                             out.data_ptr(), int(out.stride(0)), out_len.data_ptr(), C.c_void_p(st.cuda_stream)),
                  "m3_vad_log_energy")
        return out, out_len

    def decide(self, logE, lens, flags=None, threshold=None, stream=None):
        """logE (B, T) float32, lens (B,) int32 on the device -> (flags (B, T) uint8, threshold (B,) float32)"""
        c = self.cfg
        B, T = int(logE.shape[0]), int(logE.shape[1])
        self._matrix("logE", logE, torch.float32)
        self._lens("lens", lens, B)
        with torch.cuda.device(self.device), self._on(stream):
            st = torch.cuda.current_stream()
            if flags is None:
                flags = torch.empty(B, T, dtype=torch.uint8, device=self.device)
            if threshold is None:
                threshold = torch.zeros(B, dtype=torch.float32, device=self.device)
            self._matrix("flags", flags, torch.uint8, B)
            if flags.shape[1] != T or threshold.dtype != torch.float32 or threshold.numel() != B or not threshold.is_contiguous():
                raise ValueError("EnergyVad: flags must be (B, T), threshold a contiguous float32 tensor of B entries")
            check(self.lib.m3_vad_decide(logE.data_ptr(), int(logE.stride(0)), lens.data_ptr(), B, T, c.energy_threshold,
                                         c.energy_mean_scale, c.context, c.proportion_threshold, flags.data_ptr(),
                                         int(flags.stride(0)), threshold.data_ptr(), C.c_void_p(st.cuda_stream)), "m3_vad_decide")
        return flags, threshold

    def segments(self, flags, logE, lens, capacity, segments=None, n_segments=None, stream=None):
        """flags (B, T) uint8, logE (B, T) float32, lens (B,) int32 on the device -> (segments (B, capacity, 2) int32 [start, end)
        in ascending order, n_segments (B,) int32: the true count, of which only the first `capacity` are written)."""
        B, T = int(flags.shape[0]), int(flags.shape[1])
        self._matrix("flags", flags, torch.uint8)
        self._matrix("logE", logE, torch.float32, B)
        self._lens("lens", lens, B)
        capacity = int(capacity)
        if logE.shape[1] != T or capacity < 0:
            raise ValueError("EnergyVad: flags and logE must both be (B, T), capacity >= 0")
        with torch.cuda.device(self.device), self._on(stream):
            st = torch.cuda.current_stream()
            if segments is None:
                segments = torch.zeros(B, capacity, 2, dtype=torch.int32, device=self.device)
            if n_segments is None:
                n_segments = torch.zeros(B, dtype=torch.int32, device=self.device)
            if segments.dtype != torch.int32 or segments.device != self.device or tuple(segments.shape) != (B, capacity, 2) or \
                    not segments.is_contiguous():
                raise ValueError("EnergyVad: segments must be a contiguous (B, %d, 2) int32 device tensor" % capacity)
            self._lens("n_segments", n_segments, B)
            check(self.lib.m3_vad_segments(flags.data_ptr(), int(flags.stride(0)), logE.data_ptr(), int(logE.stride(0)), lens.data_ptr(),
                                           B, T, *self.cfg.segment_options(), segments.data_ptr(), capacity, n_segments.data_ptr(),
                                           C.c_void_p(st.cuda_stream)), "m3_vad_segments")
        return segments, n_segments

    def __call__(self, pcm, n_samples=None, capacity=64, stream=None, detail=False):
        """The three launches and ONE copy back (counts and lists in one buffer) -> [(start, end)] in frames per row.  A row
        with more than `capacity` segments reports its true count; the segmenter then runs once more with room for it (one
        retry, never a loop).  detail: -> (lists, logE, lens) with the device tensors of the first two launches."""
        with torch.cuda.device(self.device), self._on(stream):
            logE, lens = self.log_energy(pcm, n_samples)
            B, T = int(logE.shape[0]), int(logE.shape[1])
            if B == 0 or T == 0:
                return ([[] for _ in range(B)], logE, lens) if detail else [[] for _ in range(B)]
            flags, _ = self.decide(logE, lens)
            host = self._segments_host(flags, logE, lens, int(capacity))
            most = int(host[:, 0].max())
            if most > int(capacity):
                host = self._segments_host(flags, logE, lens, most)
            out = [[(int(s), int(e)) for s, e in host[b, 1:1 + 2 * int(host[b, 0])].view(-1, 2).tolist()] for b in range(B)]
        return (out, logE, lens) if detail else out

    def _segments_host(self, flags, logE, lens, capacity):
        B = int(flags.shape[0])
        buf = torch.zeros(B, 1 + 2 * capacity, dtype=torch.int32, device=self.device)     # count | list: one copy brings both
        seg = torch.zeros(B, capacity, 2, dtype=torch.int32, device=self.device)
        n = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.segments(flags, logE, lens, capacity, seg, n)
        buf[:, 0] = n
        buf[:, 1:] = seg.view(B, -1)
        host = buf.cpu()
        host[:, 0].clamp_(min=0)
        return host


def segment_gather(src, jobs, dst, len_out, cols=None, stream=None):
    """m3_segment_gather on device tensors: src (T_all, >= cols) float32, the features of whole recordings; jobs (B, 3) int32 =
    (src_row, start, end) per segment: rows src_row + [start, end) of src; dst (B, T_max, >= cols) float32 (e.g. an engine
    input buffer): frames behind a segment are written as zeros, columns >= cols are not touched; len_out (B,) / (1, B) int32
    receives min(end - start, T_max).  cols: default src.shape[1].  The copy is a kernel: the product path does no torch
    arithmetic.  -> dst"""
    cols = int(src.shape[1] if cols is None else cols)
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_cuda or (src.shape[1] > 1 and src.stride(1) != 1) or src.shape[1] < cols:
        raise ValueError("segment_gather: src must be a (T_all, >= %d) float32 device tensor with dense rows" % cols)
    B = int(dst.shape[0])
    if dst.dim() != 3 or dst.dtype != torch.float32 or dst.device != src.device or dst.shape[2] < cols or \
            (dst.shape[2] > 1 and dst.stride(2) != 1):
        raise ValueError("segment_gather: dst must be a (B, T_max, >= %d) float32 device tensor with dense rows" % cols)
    if jobs.dtype != torch.int32 or jobs.device != src.device or tuple(jobs.shape) != (B, 3) or not jobs.is_contiguous():
        raise ValueError("segment_gather: jobs must be a contiguous (%d, 3) int32 device tensor" % B)
    if len_out.dtype != torch.int32 or len_out.device != src.device or len_out.numel() != B or not len_out.is_contiguous():
        raise ValueError("segment_gather: len_out must be a contiguous int32 device tensor of %d entries" % B)
    with torch.cuda.device(src.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        st = torch.cuda.current_stream()
        check(_lib.load().m3_segment_gather(src.data_ptr(), int(src.stride(0)), int(src.shape[0]), jobs.data_ptr(), B,
                                            int(dst.shape[1]), cols, dst.data_ptr(), int(dst.stride(1)), int(dst.stride(0)),
                                            len_out.data_ptr(), C.c_void_p(st.cuda_stream)), "m3_segment_gather")
    return dst
