"""NumPy restatement of librosa 0.6.0's load(path, sr=16000): np.mean over the channels, then resampy's 'kaiser_best' band-limited
sinc interpolation and fix_length.  Written from the published algorithm (Smith's "Digital Audio Resampling", as resampy implements
it); neither library is needed.  Vectorised over the outputs with a loop over the taps, fp64 throughout; fp32=True accumulates the way
resampy does (fp64 weight times sample, the running sum rounded to fp32 after every tap, left wing first), which is what the GPU test's
gate is derived from.

Sample positions are t * (1 / ratio) (resampy >= 0.3); older releases add 1 / ratio up, which moves a position by about 1e-11 samples.
"""
import numpy as np

SR = 16000
NUM_ZEROS = 64
STEPS = 512                                   # table steps per zero crossing (precision 9)
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
NWIN = NUM_ZEROS * STEPS + 1                  # 32769
MAX_CHANNELS = 8

_base = None


def lengths(n, orig_sr):
    """(n_valid, n_out): the samples the interpolation writes and the length after fix_length."""
    ratio = float(SR) / orig_sr
    return int(n * ratio), int(np.ceil(n * ratio))


def base_window():
    """win[k] = rolloff * sinc(rolloff * k / 512) * I0(beta * sqrt(1 - (k / 32768)^2)) / I0(beta), k = 0..32768 (fp64, unscaled)."""
    global _base
    if _base is None:
        k = np.arange(NWIN, dtype=np.float64)
        taper = np.i0(BETA * np.sqrt(1.0 - (k / (NWIN - 1)) ** 2)) / np.i0(BETA)
        _base = ROLLOFF * np.sinc(ROLLOFF * k / STEPS) * taper
        _base.flags.writeable = False
    return _base


def filter_table(orig_sr):
    """(win, delta, index_step, scale, ratio) for orig_sr -> 16000."""
    ratio = float(SR) / orig_sr
    scale = min(1.0, ratio)
    step = int(scale * STEPS)
    win = base_window().copy()
    if ratio < 1:
        win *= ratio
    delta = np.zeros(NWIN)
    delta[:-1] = np.diff(win)
    return win, delta, step, scale, ratio


def downmix(y):
    """np.mean(y, axis=0) of float32 [C, N] spelled out: a left-to-right fp32 sum over the channels, one fp32 division by C."""
    y = np.asarray(y, dtype=np.float32)
    acc = y[0].copy()
    for c in range(1, y.shape[0]):
        acc = acc + y[c]
    return acc if y.shape[0] == 1 else acc / np.float32(y.shape[0])


def _wing(acc, x, win, delta, step, frac, first, count_cap, sign, fp32):
    idx = frac * STEPS
    off = idx.astype(np.int64)
    eta = idx - off
    count = np.minimum(count_cap, (NWIN - off) // step)
    for i in range(int(count.max()) if count.size else 0):
        m = i < count
        o = off[m] + i * step
        term = (win[o] + eta[m] * delta[o]) * x[first[m] + sign * i]
        acc[m] = (acc[m].astype(np.float64) + term).astype(np.float32) if fp32 else acc[m] + term
    return acc


def resample(x, orig_sr, fp32=False):
    """x (mono) at orig_sr -> n_out samples at 16 kHz: float64, or float32 with fp32=True.  orig_sr == 16000 returns x."""
    x32 = np.asarray(x, dtype=np.float32)
    if orig_sr == SR:
        return x32.copy() if fp32 else x32.astype(np.float64)
    x = x32.astype(np.float64)
    N = len(x)
    n_valid, n_out = lengths(N, orig_sr)
    win, delta, step, scale, ratio = filter_table(orig_sr)
    y = np.zeros(n_out, np.float32 if fp32 else np.float64)
    t = np.arange(n_valid)
    time = t * (1.0 / ratio)
    n = time.astype(np.int64)
    frac = scale * (time - n)
    acc = np.zeros(n_valid, y.dtype)
    acc = _wing(acc, x, win, delta, step, frac, n, n + 1, -1, fp32)                       # x[n - i], i < n + 1
    acc = _wing(acc, x, win, delta, step, scale - frac, n + 1, N - n - 1, +1, fp32)       # x[n + 1 + k], k < N - n - 1
    y[:n_valid] = acc
    return y


def load(y, orig_sr, fp32=False):
    """librosa.load's arithmetic on samples already read: y is float32 [N] or [N, C] (frames first, as a wav file holds them)."""
    y = np.asarray(y, dtype=np.float32)
    if y.ndim == 2:
        y = downmix(y.T)
    return resample(y, orig_sr, fp32)
