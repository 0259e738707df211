"""NumPy restatements for the prosody targets (b2s_hip.prosody, libb2s_pros.so; contracts in include/b2s_pros.h, DESIGN.md section n)
-- the oracle of tests/test_pros_host.py and tests/test_gpu_pros.py.

(a) energy(): the window energy per frame in Python integers.
(b) track(): the Viterbi search over YIN's CMND matrix, one frame at a time and vectorised over the lags.  The band is walked in
    ascending order with a strict compare and state 0 takes the first minimum (np.argmin), which is the tie rule; every fp64 product
    is rounded before it is added.  The kernel has to give these bits.
(c) contour() and units(): the continuous F0 contour and the sums per input unit; float sums go left to right (np.cumsum, never
    np.sum, which sums pairwise).
"""
import numpy as np

import f0_ref

OK, EMPTY, FAILED, SHORT, NOVOICE = 0, 1, 2, 3, 4
DEFAULTS = {"u": 0.3, "v": 0.1, "lam": 0.02, "mu": 0.0005, "W": 8}


def energy(pcm, win, hop):
    """int16 PCM of one utterance -> [1 + len // hop] int64: E[t] = sum_{i < win} p[t * hop - win // 2 + i]^2, zero outside."""
    p = np.asarray(pcm, dtype=np.int64).reshape(-1)
    L = len(p)
    F = 1 + L // hop
    out = np.zeros(F, np.int64)
    for t in range(F):
        lo = t * hop - win // 2
        seg = p[max(lo, 0):max(min(lo + win, L), 0)]
        out[t] = int(np.sum(seg * seg, dtype=np.int64))
    return out


def track(cmnd, energy, floor, tau_min, tau_max, sr=16000.0, u=0.3, v=0.1, lam=0.02, mu=0.0005, W=8):
    """cmnd [F, K] f64 (K > tau_max), energy [F] integers -> dict(tau [F] int32, f0 [F] f64, score, status, and for an OK status
    ties: the number of lag cells of ungated frames whose minimum more than one candidate holds, where the tie rule decided)."""
    c = np.asarray(cmnd, dtype=np.float64)
    F = c.shape[0]
    out = {"tau": np.zeros(F, np.int32), "f0": np.zeros(F, np.float64), "score": float("nan"), "status": FAILED}
    if F == 0:
        out.update(score=0.0, status=EMPTY)
        return out
    lags = np.arange(tau_min, tau_max + 1)
    n = len(lags)
    if not np.isfinite(c[:, tau_min:tau_max + 1]).all():
        return out
    u, v, lam, mu = (np.float64(x) for x in (u, v, lam, mu))
    bias = mu * lags.astype(np.float64)                               # rounded products
    pen = lam * np.arange(W + 1).astype(np.float64)
    gated = np.array([int(e) < int(floor) for e in energy], bool)
    inf = np.float64(np.inf)

    def loc(t):
        return np.full(n, inf) if gated[t] else c[t, tau_min:tau_max + 1] + bias
    q0, q = u, loc(0)
    back = np.zeros((F, n), np.int32)                                 # predecessor state of every lag
    back0 = np.zeros(F, np.int32)
    idx = np.arange(n)
    ties = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, F):
            cand0 = q + v
            i = int(np.argmin(cand0))                                 # the first of equal minima
            best0, arg0 = (cand0[i], tau_min + i) if cand0[i] < q0 else (q0, 0)
            best = np.full(n, q0 + v)
            arg = np.zeros(n, np.int32)
            padded = np.concatenate((np.full(W, inf), q, np.full(W, inf)))
            for j in range(-W, W + 1):                                # k' = k + j ascending
                cand = padded[idx + W + j] + pen[abs(j)]
                take = cand < best
                best = np.where(take, cand, best)
                arg = np.where(take, lags + j, arg)
            equal = (np.full(n, q0 + v) == best).astype(np.int64)    # how many candidates of a cell hold its minimum
            for j in range(-W, W + 1):
                equal += padded[idx + W + j] + pen[abs(j)] == best
            ties += int(np.sum((equal > 1) & np.isfinite(best) & ~gated[t]))
            back[t], back0[t] = arg, arg0
            q0, q = u + best0, loc(t) + best
    i = int(np.argmin(q))
    score, s = (q[i], tau_min + i) if q[i] < q0 else (q0, 0)
    for t in range(F - 1, -1, -1):
        out["tau"][t] = s
        if t > 0:
            s = int(back0[t]) if s == 0 else int(back[t, s - tau_min])
    out["f0"] = np.array([f0_ref.refine(c[t], int(out["tau"][t]), tau_max, sr) for t in range(F)], np.float64)
    out.update(score=float(score), status=OK, ties=ties)
    return out


def path_cost(cmnd, gated, states, tau_min, u, v, lam, mu):
    """The cost of one state sequence under the recurrence's own operations and order (for the brute-force test)."""
    u, v, lam, mu = (np.float64(x) for x in (u, v, lam, mu))

    def loc(t, s):
        if s == 0:
            return u
        return np.float64(np.inf) if gated[t] else np.float64(cmnd[t][s]) + mu * np.float64(s)
    cost = loc(0, states[0])
    for t in range(1, len(states)):
        a, b = states[t - 1], states[t]
        if b == 0:
            step = cost if a == 0 else cost + v
        else:
            step = cost + v if a == 0 else cost + lam * np.float64(abs(a - b))
        cost = loc(t, b) + step
    return cost


def contour(f0, tau, n):
    """The continuous contour over the first n frames of f0 / tau (0 from n on), or None without a voiced frame among them."""
    f0 = np.asarray(f0, dtype=np.float64)
    out = np.zeros(len(f0), np.float64)
    voiced = np.nonzero(np.asarray(tau[:n]) > 0)[0]
    if len(voiced) == 0:
        return None
    for t in range(n):
        i = int(np.searchsorted(voiced, t))                           # voiced[i] is the first voiced frame at or after t
        if i < len(voiced) and voiced[i] == t:
            out[t] = f0[t]
        elif i == 0:
            out[t] = f0[voiced[0]]
        elif i == len(voiced):
            out[t] = f0[voiced[-1]]
        else:
            a, b = int(voiced[i - 1]), int(voiced[i])
            out[t] = f0[a] + (f0[b] - f0[a]) * (np.float64(t - a) / np.float64(b - a))
    return out


def _left_to_right(x):
    return float(np.cumsum(np.asarray(x, dtype=np.float64))[-1]) if len(x) else 0.0


def units(f0, tau, energy, durations, n_in, groups=None):
    """One utterance: f0 / tau / energy [F], durations [S], n_in = input length, groups [S] or None.  -> dict(cont [F], frames,
    voiced [S] int32, f0_voiced_sum, f0_cont_sum [S] f64, energy_sum [S] int64, units, status)."""
    F, S = len(f0), len(durations)
    out = {"cont": np.zeros(F, np.float64), "frames": np.zeros(S, np.int32), "voiced": np.zeros(S, np.int32),
           "f0_voiced_sum": np.zeros(S, np.float64), "f0_cont_sum": np.zeros(S, np.float64), "energy_sum": np.zeros(S, np.int64),
           "units": 0, "status": FAILED}
    if not 0 <= n_in <= S:
        return out
    if n_in == 0:
        out["status"] = EMPTY
        return out
    d = [int(x) for x in durations[:n_in]]
    g = list(range(n_in)) if groups is None else [int(x) for x in groups[:n_in]]
    if min(d) < 0 or g[0] != 0 or any(not 0 <= b - a <= 1 for a, b in zip(g, g[1:])):
        return out
    n = sum(d)
    if n > F:
        out["status"] = SHORT
        return out
    cont = contour(f0, tau, n)
    out["status"] = OK if cont is not None else NOVOICE
    if cont is not None:
        out["cont"] = cont
    out["units"] = g[-1] + 1
    tau = np.asarray(tau)
    pos = 0
    per_unit = [0] * out["units"]
    for i in range(n_in):
        per_unit[g[i]] += d[i]
    for j, m in enumerate(per_unit):
        fr = np.arange(pos, pos + m)
        vo = fr[tau[fr] > 0] if m else fr
        out["frames"][j], out["voiced"][j] = m, len(vo)
        out["f0_voiced_sum"][j] = _left_to_right(np.asarray(f0)[vo])
        out["f0_cont_sum"][j] = _left_to_right(out["cont"][fr])
        out["energy_sum"][j] = sum(int(energy[t]) for t in fr)
        pos += m
    return out


def means(res):
    """pitch, pitch_voiced, energy per unit as the module derives them: fp64 quotients, 0 where the denominator is 0."""
    fr, vo = res["frames"].astype(np.float64), res["voiced"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"pitch": np.where(fr > 0, res["f0_cont_sum"] / fr, 0.0), "pitch_voiced": np.where(vo > 0, res["f0_voiced_sum"] / vo, 0.0),
                "energy": np.where(fr > 0, res["energy_sum"].astype(np.float64) / fr, 0.0)}


def planted_signal():
    """The glide of the planted-track test: 12 000 samples at 16 kHz, 110 -> 190 Hz with three harmonics, a pause at 4000..5600 and
    noise from 7000 on.  -> (fp32 waveform, the frequency per sample)."""
    sr, n = 16000, 12000
    f = np.linspace(110.0, 190.0, n)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = 0.5 * (np.sin(ph) + 0.9 * np.sin(2 * ph + 1) + 0.4 * np.sin(3 * ph))
    x[4000:5600] = 0
    rng = np.random.default_rng(1)
    x[7000:] += 0.25 * rng.standard_normal(n - 7000)
    return x.astype(np.float32), f
