"""NumPy restatement of the YIN pitch tracker and the F0 error along a DTW path (DESIGN.md section l) -- the oracle of
tests/test_f0_host.py and tests/test_gpu_f0.py, written from de Cheveigne & Kawahara (2002), steps 1 to 5.

The difference function d and its running sum S are int64 / Python integers, so nothing about them rounds; c[tau] is the single
fp64 division float(d[tau] * tau) / float(S[tau]); the refinement is plain fp64.  The GPU result has to equal this bit for bit."""
import math

import numpy as np

OK, EMPTY, FAILED = 0, 1, 2


def quantize(wav):
    """fp32 samples -> (int16 PCM by the rule of save_wav, peak, status).  A non-finite sample: zeros, peak 0 and FAILED."""
    wav = np.asarray(wav, dtype=np.float32).reshape(-1)
    if not np.all(np.isfinite(wav)):
        return np.zeros(len(wav), np.int16), np.float32(0), FAILED
    peak = np.max(np.abs(wav)) if len(wav) else np.float32(0)
    scaled = wav.astype(np.float64) / max(0.01, float(peak))
    return np.rint(np.clip(scaled, -1.0, 1.0) * 32767).astype(np.int16), np.float32(peak), OK


def min_energy(win, silence_db):
    """The energy floor of a frame as a Python int: a window of `win` samples at silence_db below full scale; None: 0."""
    if silence_db is None:
        return 0
    return int(math.ceil(win * (32767.0 * 10.0 ** (silence_db / 20.0)) ** 2))


def segment(pcm, t, win, hop, tau_max):
    """seg[i] = pcm[t * hop - (win + tau_max) // 2 + i], i < win + tau_max, zero outside the signal; int64."""
    n = win + tau_max
    first = t * hop - n // 2
    idx = first + np.arange(n)
    inside = (idx >= 0) & (idx < len(pcm))
    seg = np.zeros(n, np.int64)
    seg[inside] = np.asarray(pcm, dtype=np.int64)[idx[inside]]
    return seg


def difference(seg, win, tau_max):
    """d[tau] = sum_{j < win} (seg[j] - seg[j + tau])^2, tau = 0..tau_max, exact in int64 (below 2^43)."""
    shifted = np.lib.stride_tricks.sliding_window_view(seg, win)[:tau_max + 1]         # [tau, j] = seg[j + tau]
    e = seg[None, :win] - shifted
    return np.sum(e * e, axis=1, dtype=np.int64)


def cmnd(d):
    """c[0] = 1; c[tau] = 1 when S[tau] = d[1] + .. + d[tau] is 0, else float(d[tau] * tau) / float(S[tau])."""
    c = np.ones(len(d), np.float64)
    S = 0
    for tau in range(1, len(d)):
        S += int(d[tau])
        if S != 0:
            c[tau] = np.float64(float(int(d[tau]) * tau)) / np.float64(float(S))
    return c


def pick(c, energy, tau_min, tau_max, threshold, floor):
    """The lag of the frame, 0 for unvoiced."""
    if energy < floor:
        return 0
    below = [k for k in range(tau_min, tau_max + 1) if c[k] < threshold]
    if not below:
        return 0
    k = below[0]
    while k + 1 <= tau_max and c[k + 1] < c[k]:
        k += 1
    return k


def refine(c, tau, tau_max, sr):
    if tau == 0:
        return 0.0
    shift = np.float64(0.0)
    if tau - 1 >= 1 and tau + 1 <= tau_max:
        a, b, cc = c[tau - 1], c[tau], c[tau + 1]
        den = (a - b) + (cc - b)
        if den > 0:
            s = np.float64(0.5) * (a - cc) / den
            if abs(s) <= 1:
                shift = s
    return float(np.float64(sr) / (np.float64(tau) + shift))


def yin(pcm, win=800, hop=200, tau_min=32, tau_max=266, threshold=0.1, floor=0, sr=16000.0):
    """int16 PCM of one utterance -> dict(f0 [F] f64, tau [F] int32, aper [F] f64, cmnd [F, tau_max + 1] f64, energy [F] ints),
    F = 1 + len // hop."""
    pcm = np.asarray(pcm)
    F = 1 + len(pcm) // hop
    f0, tau, aper = np.zeros(F, np.float64), np.zeros(F, np.int32), np.zeros(F, np.float64)
    cm = np.zeros((F, tau_max + 1), np.float64)
    energy = []
    for t in range(F):
        seg = segment(pcm, t, win, hop, tau_max)
        c = cmnd(difference(seg, win, tau_max))
        e = int(np.sum(seg[:win] * seg[:win], dtype=np.int64))
        k = pick(c, e, tau_min, tau_max, threshold, floor)
        cm[t], aper[t], tau[t], f0[t] = c, np.min(c[tau_min:tau_max + 1]), k, refine(c, k, tau_max, sr)
        energy.append(e)
    return {"f0": f0, "tau": tau, "aper": aper, "cmnd": cm, "energy": energy}


def score(f0_x, tau_x, f0_y, tau_y, kept_x, kept_y, path, gross_ratio=0.2):
    """x the prediction, y the target; path: (i, j) over kept frames, kept_x / kept_y: kept frame -> frame number.  Returns
    dict(status, counts = [steps, vuv, both, gross], scores = [rmse_hz, rmse_cents, vde, gpe, ffe])."""
    nan = float("nan")
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    if len(path) == 0:
        return {"status": EMPTY, "counts": [0, 0, 0, 0], "scores": [nan] * 5}
    failed = {"status": FAILED, "counts": [0, 0, 0, 0], "scores": [nan] * 5}
    if path[:, 0].min() < 0 or path[:, 0].max() >= len(kept_x) or path[:, 1].min() < 0 or path[:, 1].max() >= len(kept_y):
        return failed
    fi, fj = np.asarray(kept_x, dtype=np.int64)[path[:, 0]], np.asarray(kept_y, dtype=np.int64)[path[:, 1]]
    if fi.min() < 0 or fi.max() >= len(f0_x) or fj.min() < 0 or fj.max() >= len(f0_y):
        return failed
    vx, vy = np.asarray(tau_x)[fi] > 0, np.asarray(tau_y)[fj] > 0
    both = vx & vy
    x, y = np.asarray(f0_x, dtype=np.float64)[fi][both], np.asarray(f0_y, dtype=np.float64)[fj][both]
    steps, vuv, nb = len(path), int(np.sum(vx != vy)), int(np.sum(both))
    gross = int(np.sum(np.abs(x - y) > np.float64(gross_ratio) * y))
    cents = 1200.0 * np.log2(x / y)
    return {"status": OK, "counts": [steps, vuv, nb, gross],
            "scores": [math.sqrt(float(np.sum((x - y) ** 2)) / nb) if nb else nan,
                       math.sqrt(float(np.sum(cents ** 2)) / nb) if nb else nan,
                       vuv / steps, gross / nb if nb else nan, (vuv + gross) / steps]}
