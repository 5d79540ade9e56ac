"""Reference for the log-Mel filter bank tests (a helper, not a test): the front end's contract restated in numpy from its
formulas, independently of m3asr/frontend.py and of the library's tables.

Kaldi compute-fbank-feats with the options of a served model: 16 kHz, frames of 400 samples every 160 (snip_edges), per frame
subtract the mean, pre-emphasis 0.97, Povey window, zero-pad to 512, power spectrum of bins 0..255 (no Nyquist bin), triangular
mel filters between 20 Hz and Nyquist with weights taken in the mel domain (both edges open), log(max(E, FLT_EPSILON)).

fbank_ref(pcm, bins)             float64 throughout (numpy.fft.rfft)
fbank_ref(pcm, bins, np.float32) the same evaluation in float32 throughout (scipy.fft.rfft keeps float32): its distance to
                                 the float64 result is the yardstick for what a correct float32 implementation may differ by
"""
import numpy as np

FRAME, SHIFT, NFFT, RATE, LOW_FREQ = 400, 160, 512, 16000.0, 20.0
FLT_EPSILON = float(np.finfo(np.float32).eps)
LOG_FLOOR = np.float32(np.log(np.float64(FLT_EPSILON)))


def num_frames(n):
    return 0 if n < FRAME else 1 + (n - FRAME) // SHIFT


def povey_window():
    i = np.arange(FRAME, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FRAME - 1))) ** 0.85


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_weights(bins):
    """(bins, 256) float64: weight of FFT bin j in mel bin m."""
    lo, hi = mel(LOW_FREQ), mel(RATE / 2)
    delta = (hi - lo) / (bins + 1)
    mj = mel(np.arange(NFFT // 2) * RATE / NFFT)
    w = np.zeros((bins, NFFT // 2))
    for m in range(bins):
        left, centre, right = lo + m * delta, lo + (m + 1) * delta, lo + (m + 2) * delta
        up, down = (mj - left) / (centre - left), (right - mj) / (right - centre)
        inside = (mj > left) & (mj < right)
        w[m] = np.where(inside, np.where(mj <= centre, up, down), 0.0)
    return w


def energies(pcm, bins=40, dtype=np.float64):
    """Mel energies (frames, bins) of one signal, before the floor and the log, evaluated in `dtype`."""
    x = np.asarray(pcm).astype(dtype).reshape(-1)
    nf = num_frames(x.shape[0])
    if nf == 0:
        return np.zeros((0, bins), dtype=dtype)
    idx = SHIFT * np.arange(nf)[:, None] + np.arange(FRAME)[None, :]
    fr = x[idx]
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr - dtype(0.97) * prev
    fr = fr * povey_window().astype(dtype)
    padded = np.zeros((nf, NFFT), dtype=dtype)
    padded[:, :FRAME] = fr
    if dtype == np.float64:
        spec = np.fft.rfft(padded, axis=1)
    else:
        import scipy.fft
        spec = scipy.fft.rfft(padded, axis=1)
        assert spec.dtype == np.complex64
    power = (spec.real * spec.real + spec.imag * spec.imag)[:, :NFFT // 2].astype(dtype)
    out = power @ mel_weights(bins).astype(dtype).T
    assert out.dtype == dtype
    return out


def fbank_ref(pcm, bins=40, dtype=np.float64):
    """log-Mel features (frames, bins) of one signal in `dtype`."""
    e = energies(pcm, bins, dtype)
    return np.log(np.maximum(e, dtype(FLT_EPSILON)))
