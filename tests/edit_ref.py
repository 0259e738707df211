"""Host restatements of the edit-distance contract of b2s_met_edit_distance (include/b2s_metrics.h), for the CER tests.

Unit costs; per pair the lexicographically smallest (cost, substitutions) over all alignments of truth `a` and prediction `b`.  A
deletion is a truth symbol missing from the prediction, an insertion the reverse, so del - ins = len(a) - len(b).

    edit_tuples(a, b)   pure-Python DP over (cost, sub, del, ins) tuples: the contract spelled out, slow
    edit_packed(a, b)   NumPy, one row at a time on packed int64 cells cost << 16 | sub: a mismatch on the diagonal adds 0x10001, a
                        match 0, a deletion or insertion 0x10000; cand = min(diag, up), and the left-to-right chain
                        row[j] = min(cand[j], row[j - 1] + 0x10000) is minimum.accumulate of cand - (j << 16), plus (j << 16)

Both return (cost, sub, del, ins) as Python ints.  cer(d, n_pred) is the reference's score expression.
"""
import numpy as np

D = 1 << 16


def edit_tuples(a, b):
    a, b = list(a), list(b)
    prev = [(j, 0, 0, j) for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        row = [(i, 0, i, 0)]
        for j in range(1, len(b) + 1):
            c, s, d, n = prev[j - 1]
            diag = (c, s, d, n) if a[i - 1] == b[j - 1] else (c + 1, s + 1, d, n)
            c, s, d, n = prev[j]
            up = (c + 1, s, d + 1, n)
            c, s, d, n = row[j - 1]
            left = (c + 1, s, d, n + 1)
            row.append(min((diag, up, left), key=lambda v: (v[0], v[1])))
        prev = row
    return prev[len(b)]


def breakdown(packed, la, lb):
    cost, sub = int(packed) >> 16, int(packed) & 0xFFFF
    dele = (cost - sub + la - lb) // 2
    return cost, sub, dele, cost - sub - dele


def edit_packed(a, b):
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    la, lb = len(a), len(b)
    shift = np.arange(lb + 1, dtype=np.int64) * D
    row = shift.copy()
    for i in range(la):
        cand = np.empty(lb + 1, dtype=np.int64)
        cand[0] = (i + 1) * D
        np.minimum(row[:-1] + (a[i] != b) * (D + 1), row[1:] + D, out=cand[1:])
        row = np.minimum.accumulate(cand - shift) + shift
    return breakdown(row[lb], la, lb)


def cer(d, n_pred):
    return min(1.0, d / (n_pred + 1e-9))


def mutate(rng, seq, rate, alphabet):
    """`seq` with about `rate` random edits per symbol (substitution, deletion or insertion, equally likely)."""
    out = []
    for v in seq:
        r = rng.random()
        if r < rate / 3:
            out.append(int(rng.integers(alphabet)))
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out.extend((int(v), int(rng.integers(alphabet))))
        else:
            out.append(int(v))
    return np.asarray(out, dtype=np.int32)
