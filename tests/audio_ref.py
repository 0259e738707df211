"""fp64 NumPy/SciPy restatement of the reference's utils/audio.py (librosa 0.6.0 semantics) -- the oracle of the vocoder tests
and what `bench_vocoder.py --cpu-baseline` times.  Not a test module (no test_ prefix), a helper like tests/gpu_util.py.

Parameters are the package's `_SIGNAL` hyper-parameters: sr 16000, n_fft 2048, hop 200, win 800, 80 mels, preemphasis 0.97,
ref_db 20, max_db 100, max_abs_value 4, symmetric mel, n_iter 60, power 1.5.
"""
import numpy as np
from scipy import signal

SR, N_FFT, HOP, WIN, N_MELS = 16000, 2048, 200, 800, 80
PREEMPH, REF_DB, MAX_DB, MAX_ABS, POWER, N_ITER = 0.97, 20.0, 100.0, 4.0, 1.5, 60
TINY32 = float(np.finfo(np.float32).tiny)


def window():
    """Periodic Hann of length WIN, zero-padded to N_FFT centred (librosa pad_center): 624 zeros in front."""
    n = np.arange(WIN)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / WIN)
    lpad = (N_FFT - WIN) // 2
    return np.concatenate([np.zeros(lpad), w, np.zeros(N_FFT - WIN - lpad)])


def hz_to_mel(f):
    """Slaney mel scale: linear below 1 kHz (200/3 Hz per mel), logarithmic above (step ln(6.4)/27)."""
    f = np.asanyarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    mels = f / f_sp
    min_log_mel = min_log_hz / f_sp
    log_t = f >= min_log_hz
    mels = np.where(log_t, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, mels)
    return mels


def mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_basis(sr=SR, n_fft=N_FFT, n_mels=N_MELS):
    """librosa.filters.mel(sr, n_fft, n_mels), htk=False, norm=1: [n_mels, 1 + n_fft // 2] float64."""
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights


def reflect_index(i, n):
    """NumPy 'reflect' padding index (no edge repeat), including the repeated reflection of a pad longer than the signal."""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def stft(y):
    """librosa.stft(y, 2048, 200, 800), center=True, pad_mode='reflect': [1025, 1 + len(y) // 200] complex128."""
    y = np.asarray(y, dtype=np.float64)
    yp = np.pad(y, N_FFT // 2, mode="reflect")
    n_frames = 1 + (len(yp) - N_FFT) // HOP
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(n_frames)[:, None]
    frames = yp[idx] * window()[None, :]
    return np.fft.rfft(frames, axis=1).T


def istft(X):
    """librosa.istft(X, 200, 800, window='hann'), center=True: length 200 * (T - 1) float64."""
    X = np.asarray(X)
    T = X.shape[1]
    w = window()
    frames = np.fft.irfft(X.T, n=N_FFT, axis=1) * w[None, :]
    n = N_FFT + HOP * (T - 1)
    y = np.zeros(n)
    wss = np.zeros(n)
    for t in range(T):
        y[t * HOP:t * HOP + N_FFT] += frames[t]
        wss[t * HOP:t * HOP + N_FFT] += w * w
    nz = wss > TINY32
    y[nz] /= wss[nz]
    return y[N_FFT // 2:-(N_FFT // 2)]


_inv_basis = None


def inverse_mel_basis():
    global _inv_basis
    if _inv_basis is None:
        _inv_basis = np.linalg.pinv(mel_basis())
    return _inv_basis


def mel_to_mag(mel, power=POWER):
    """Normalised mel [T, 80] -> S = max(1e-10, pinv @ amp) ** power, [1025, T] float64."""
    m = (np.asarray(mel, dtype=np.float64).T + MAX_ABS) / (2 * MAX_ABS)
    m = np.clip(m, 0, 1) * MAX_DB - MAX_DB + REF_DB
    amp = np.power(10.0, m * 0.05)
    return np.maximum(1e-10, inverse_mel_basis() @ amp) ** power


def griffin_lim(S, n_iter=N_ITER):
    """Returns y before de-emphasis."""
    X = S.astype(np.complex128)
    for _ in range(n_iter):
        est = stft(istft(X))
        X = S * est / np.maximum(1e-8, np.abs(est))
    return istft(X)


def deemphasis(y):
    return signal.lfilter([1], [1, -PREEMPH], y)


def mel2wav(mel, n_iter=N_ITER, return_raw=False):
    """The reference's mel2wav: float32 wav of length 200 * (T - 1).  With return_raw, also y before de-emphasis and S."""
    S = mel_to_mag(mel)
    y = griffin_lim(S, n_iter)
    wav = deemphasis(y).astype(np.float32)
    return (wav, y, S) if return_raw else wav


def spectral_convergence(y, S):
    """|| |stft(y)| - S || / || S || (y before de-emphasis)."""
    return float(np.linalg.norm(np.abs(stft(y)) - S) / np.linalg.norm(S))


def get_spectrograms(wav):
    """The reference's get_spectrograms: normalised mel [1 + len // 200, 80] float32."""
    y = np.asarray(wav, dtype=np.float64)
    y = np.append(y[0], y[1:] - PREEMPH * y[:-1])
    mag = np.abs(stft(y))
    mel = mel_basis() @ mag
    mel = 20 * np.log10(np.maximum(1e-5, mel))
    mel = np.clip((mel - REF_DB + MAX_DB) / MAX_DB, 1e-8, 1)
    mel = mel * MAX_ABS * 2 - MAX_ABS
    return mel.T.astype(np.float32)
