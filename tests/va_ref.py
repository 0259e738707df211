"""NumPy restatement of libb2s_va.so (include/b2s_va.h, DESIGN.md section o): quantise, frames, forward and backward of the variance
adaptor, one utterance or one batch at a time, in the order the definition gives.  Every fp32 sum is an explicit loop of rounded
additions, acc = (acc + row).astype(np.float32); np.sum adds pairwise and is never used on fp32 here.  Not fast, not meant to be."""
import numpy as np

OK, EMPTY, FAILED = 0, 1, 2
MAX_S, MAX_D, MAX_BINS, MAX_FRAMES = 1024, 1024, 256, 1 << 20
F32 = np.float32


def boundaries_ok(boundaries):
    b = np.asarray(boundaries, np.float64).reshape(-1)
    return bool(np.all(np.isfinite(b)) and np.all(b[1:] > b[:-1]))


def quantise(values, input_lengths, boundaries):
    """values [B, S] f64 -> (bins [B, S] int32, status [B] int32): the count of boundaries strictly below each value."""
    v = np.asarray(values, np.float64)
    bd = np.zeros(0) if boundaries is None else np.asarray(boundaries, np.float64).reshape(-1)
    B, S = v.shape
    bins, status = np.zeros((B, S), np.int32), np.zeros(B, np.int32)
    good = boundaries_ok(bd)
    for b in range(B):
        n = int(input_lengths[b])
        if not good or n < 0 or n > S or np.isnan(v[b, :n]).any():
            status[b] = FAILED
            continue
        status[b] = EMPTY if n == 0 else OK
        for s in range(n):
            bins[b, s] = sum(1 for x in bd if x < v[b, s])
    return bins, status


def frames(durations, input_lengths):
    """durations [B, S] -> (frames [B] int32, status [B] int32)."""
    d = np.asarray(durations)
    B, S = d.shape
    out, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        n = int(input_lengths[b])
        if n < 0 or n > S or (d[b, :n] < 0).any() or int(d[b, :n].astype(np.int64).sum()) > MAX_FRAMES:
            status[b] = FAILED
            continue
        status[b] = EMPTY if n == 0 else OK
        out[b] = int(d[b, :n].astype(np.int64).sum())
    return out, status


def utterance_status(n, S, dur, bins_list, n_bins, o0, o1, total):
    """The status word forward and backward give one utterance."""
    if n < 0 or n > S:
        return FAILED
    d = np.asarray(dur[:n]).astype(np.int64)
    if (d < 0).any() or int(d.sum()) > MAX_FRAMES:
        return FAILED
    for bn in bins_list:
        if bn is not None and ((np.asarray(bn[:n]) < 0).any() or (np.asarray(bn[:n]) >= n_bins).any()):
            return FAILED
    if o0 < 0 or o1 < o0 or o1 > total or o1 - o0 != int(d.sum()):
        return FAILED
    return EMPTY if n == 0 else OK


def statuses(pb, eb, n_bins, dur, input_lengths, off, total):
    B, S = np.asarray(dur).shape
    return np.array([utterance_status(int(input_lengths[b]), S, dur[b], [None if pb is None else pb[b], None if eb is None else eb[b]],
                                      n_bins, int(off[b]), int(off[b + 1]), total) for b in range(B)], np.int32)


def forward(x, pb, eb, pt, et, dur, input_lengths, off, total, sentinel=np.nan):
    """-> dict h [B, S, D], y [total, D], unit_of_frame [total], status [B].  What the call does not write holds `sentinel` (h, y) or
    -1 (unit_of_frame)."""
    x = np.asarray(x, F32)
    B, S, D = x.shape
    n_bins = (pt if pt is not None else et if et is not None else np.zeros((1, D))).shape[0]
    st = statuses(pb, eb, n_bins, dur, input_lengths, off, total)
    h = np.full((B, S, D), sentinel, F32)
    y = np.full((total, D), sentinel, F32)
    uof = np.full(total, -1, np.int32)
    for b in range(B):
        if st[b] == FAILED:
            continue
        n = int(input_lengths[b])
        h[b] = F32(0.0)
        t = int(off[b])
        for s in range(n):
            row = x[b, s]
            if pt is not None:
                row = (row + pt[pb[b, s]]).astype(F32)
            if et is not None:
                row = (row + et[eb[b, s]]).astype(F32)
            h[b, s] = row
            for _ in range(int(dur[b][s])):
                y[t] = row
                uof[t] = s
                t += 1
    return {"h": h, "y": y, "unit_of_frame": uof, "status": st}


def backward(dy, pb, eb, n_bins, dur, input_lengths, off, total, D=None):
    """-> dict dx [B, S, D], d_pitch_table, d_energy_table [n_bins, D] (None without the bins), status [B]."""
    dy = np.asarray(dy, F32)
    D = dy.shape[1] if D is None else D
    B, S = np.asarray(dur).shape
    st = statuses(pb, eb, n_bins, dur, input_lengths, off, total)
    dx = np.zeros((B, S, D), F32)
    for b in range(B):
        if st[b] != OK:
            continue
        t = int(off[b])
        for s in range(int(input_lengths[b])):
            acc = np.zeros(D, F32)
            for _ in range(int(dur[b][s])):
                acc = (acc + dy[t]).astype(F32)
                t += 1
            dx[b, s] = acc
    tables = []
    for bins in (pb, eb):
        if bins is None:
            tables.append(None)
            continue
        dt = np.zeros((n_bins, D), F32)
        for b in range(B):
            if st[b] != OK:
                continue
            part = np.zeros((n_bins, D), F32)
            for s in range(int(input_lengths[b])):
                k = int(bins[b, s])
                part[k] = (part[k] + dx[b, s]).astype(F32)
            for k in range(n_bins):
                dt[k] = (dt[k] + part[k]).astype(F32)
        tables.append(dt)
    return {"dx": dx, "d_pitch_table": tables[0], "d_energy_table": tables[1], "status": st}


def offsets(durations, input_lengths):
    """B + 1 int32 offsets of the frames the durations ask for (a length outside 0..S counts as 0 frames)."""
    d = np.asarray(durations)
    fr = [int(d[b, :n].astype(np.int64).sum()) if 0 <= n <= d.shape[1] else 0 for b, n in enumerate(int(v) for v in input_lengths)]
    return np.concatenate([[0], np.cumsum(fr)]).astype(np.int32)


def bits(a):
    """fp32 array -> its int32 bit patterns (what the GPU tests compare)."""
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)
