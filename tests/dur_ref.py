"""NumPy restatements for the duration feature (b2s_hip.durations, libb2s_dur.so; contracts in include/b2s_dur.h).

(a) mas(): the monotonic alignment search exactly as DESIGN.md section (m) defines it, in fp64, one frame at a time and vectorised
    over the encoder positions: Q[0][0] = p[0][0], Q[0][s > 0] = -inf, Q[t][s] = p[s][t] + max(Q[t-1][s], Q[t-1][s-1]),
    move[t][s] = Q[t-1][s-1] > Q[t-1][s] (strict), and the walk back from (Tb - 1, Sb - 1).  Every cell is one add and one compare,
    so there is nothing for the kernel to round differently: it has to give these bits.
(b) counts(): the twelve integers of b2s_dur_score in Python integers.

staircase() plants a known duration vector into a map; the host tests, the GPU tests and bench_dur.py share it.
"""
import numpy as np

OK, EMPTY, FAILED, SHORT = 0, 1, 2, 3
N_COUNTS = 12


def mas(p, Sb, Tb):
    """p: [S, T] fp32 map of one utterance.  Returns a dict: path [T] int32 (-1 from Tb on), durations [S] int32 (0 from Sb on),
    score (float, fp64) and status."""
    p = np.asarray(p)
    S, T = p.shape
    out = {"path": np.full(T, -1, np.int32), "durations": np.zeros(S, np.int32), "score": float("nan"), "status": FAILED}
    if not (0 <= Sb <= S and 0 <= Tb <= T):
        return out
    if Sb == 0 or Tb == 0:
        out.update(score=0.0, status=EMPTY)
        return out
    if Tb < Sb:
        out["status"] = SHORT
        return out
    w = p[:Sb, :Tb].astype(np.float64)                       # exact
    if not np.isfinite(w).all():
        return out
    Q = np.full(Sb, -np.inf)
    Q[0] = w[0, 0]
    moves = np.zeros((Tb, Sb), bool)
    for t in range(1, Tb):
        left = np.concatenate(([-np.inf], Q[:-1]))
        moves[t] = left > Q
        Q = w[:, t] + np.maximum(Q, left)
    s = Sb - 1
    for t in range(Tb - 1, -1, -1):
        out["path"][t] = s
        if t > 0 and moves[t, s]:
            s -= 1
    out["durations"][:Sb] = np.bincount(out["path"][:Tb], minlength=Sb)
    out.update(score=float(Q[Sb - 1]), status=OK)
    return out


def mas_batch(maps, enc_len, dec_len):
    """maps [B, S, T] -> path [B, T], durations [B, S], score [B] f64, status [B] int32."""
    res = [mas(maps[b], int(enc_len[b]), int(dec_len[b])) for b in range(len(maps))]
    return {"path": np.stack([r["path"] for r in res]), "durations": np.stack([r["durations"] for r in res]),
            "score": np.array([r["score"] for r in res], np.float64), "status": np.array([r["status"] for r in res], np.int32)}


def counts(dx, dy, n, groups=None):
    """One pair: dx, dy [S] integers, n = enc_len, groups [S] or None.  -> (twelve Python ints, status)."""
    S = len(dx)
    zero = [0] * N_COUNTS
    if not 0 <= n <= S:
        return zero, FAILED
    if n == 0:
        return zero, EMPTY
    x, y = [int(v) for v in dx[:n]], [int(v) for v in dy[:n]]
    g = list(range(n)) if groups is None else [int(v) for v in groups[:n]]
    if min(x) < 0 or min(y) < 0 or g[0] != 0 or any(not 0 <= b - a <= 1 for a, b in zip(g, g[1:])):
        return zero, FAILED
    if sum(x) > 2 ** 31 - 1 or sum(y) > 2 ** 31 - 1:
        return zero, FAILED
    ux, uy = [0] * (g[-1] + 1), [0] * (g[-1] + 1)
    for i in range(n):
        ux[g[i]] += x[i]
        uy[g[i]] += y[i]
    return [len(ux), sum(ux), sum(uy), sum(abs(a - b) for a, b in zip(ux, uy)), sum((a - b) ** 2 for a, b in zip(ux, uy)),
            sum(a * a for a in ux), sum(b * b for b in uy), sum(a * b for a, b in zip(ux, uy)), max(ux), max(uy),
            sum(a == 0 for a in ux), sum(b == 0 for b in uy)], OK


def counts_batch(dur_x, dur_y, enc_len, groups=None):
    """-> counts [B, 12] int64, status [B] int32."""
    res = [counts(dur_x[b], dur_y[b], int(enc_len[b]), None if groups is None else groups[b]) for b in range(len(dur_x))]
    return np.array([r[0] for r in res], np.int64).reshape(len(res), N_COUNTS), np.array([r[1] for r in res], np.int32)


def code_point_groups(ids, n):
    """Unit ids of the first n byte ids of utils/text.py: a UTF-8 continuation byte (0x80..0xBF) joins the byte before it."""
    out, unit = [], -1
    for i in range(n):
        if i == 0 or not 0x80 <= int(ids[i]) <= 0xBF:
            unit += 1
        out.append(unit)
    return out


def random_durations(rng, S, T):
    """S integers >= 1 that sum to T (T >= S), drawn by cutting 0..T at S - 1 distinct places."""
    cuts = np.sort(rng.choice(np.arange(1, T), size=S - 1, replace=False)) if S > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate(([0], cuts, [T]))).astype(np.int64)


def staircase(rng, durations, noise=0.2, weight=1.0):
    """[S, T] fp32: uniform noise in [0, noise) with `weight` added along the staircase that gives position s durations[s] frames.
    With noise < weight a path loses on every frame where it leaves the staircase (there it collects less than `noise`, the
    staircase at least `weight`) and gains nowhere, so the search has to return these durations."""
    S, T = len(durations), int(np.sum(durations))
    p = (rng.random((S, T)) * noise).astype(np.float32)
    p[np.repeat(np.arange(S), durations), np.arange(T)] += np.float32(weight)
    return p
