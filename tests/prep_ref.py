"""NumPy restatement, with explicit dtypes, of the body of the reference's corpora/process_corpus.py trim_audios (lines 44-116), built on
tests/silence_ref.py's split / trim_index -- the oracle of the corpus-preparation tests and what `bench_prep.py --cpu-baseline` times.
Not a test module (no test_ prefix), a helper like tests/silence_ref.py; it also holds the fixture signals.

librosa is not available where these tests run, so there is no recorded golden: the restatement is pinned by analytic cases in
tests/test_prep_host.py, where the answer follows by hand.

Arithmetic, stated with dtypes so that it does not depend on the NumPy version installed (the reference ran under NumPy 1.x):
    ref, mv         fp32 maxima of |y|;  ref / 10 and ref / 4 are fp32 quotients
    v95             np.sort(np.abs(voiced))[int(len(voiced) * 0.95)], an fp32 sample
    scale           fp32(fp64(0.244) / fp64(v95)) -- NumPy 1.x divides a Python float by an fp32 scalar in fp64 ...
    y2              y * scale in fp32            -- ... and an fp32 array times that scalar stays fp32
    out             float32; the reference's zero padding is np.zeros (fp64), which only changes the dtype of the file, not a value
Status: 0 ok, 1 gap, 2 length, 3 silent (ref == 0 or v95 == 0; the reference divides by zero there).  Precedence gap, silent, length.
"""
import functools

import numpy as np

import silence_ref as S

OK, GAP, LENGTH, SILENT = 0, 1, 2, 3
SPLIT1, SPLIT2 = (40, 2048, 512), (40, 256, 64)
assert S.PARAM_SETS[1:] == [SPLIT1, SPLIT2]
LEAD, TAIL, MIN_OUT, MAX_OUT, SPIKE_GAP = 1600, 2400, 16000, 320000, 4096
FLOOR = 3e-5


def abs_quantile(y, intervals, fraction):
    """The k-th smallest |y| over the samples of the intervals, k = min(int(N * fraction), N - 1); 0.0 if N == 0."""
    y = np.asarray(y, np.float32)
    parts = [y[s:e] for s, e in intervals]
    v = np.sort(np.abs(np.concatenate(parts))) if parts else np.zeros(0, np.float32)
    if v.size == 0:
        return np.float32(0)
    return v[min(int(v.size * fraction), v.size - 1)]


def select_intervals(y, ints):
    """The reference's two `while` loops: (kept intervals, n_removed)."""
    ints = [(int(a), int(b)) for a, b in ints]
    y_abs = np.abs(np.asarray(y, np.float32))
    ref = np.float32(y_abs.max())
    tenth, quarter = np.float32(ref / np.float32(10)), np.float32(ref / np.float32(4))
    n_removed = 0
    while len(ints) > 1:
        if ints[0][0] == ints[0][1]:
            ints = ints[1:]
            n_removed += 1
            continue
        mv = np.float32(y_abs[ints[0][0]:ints[0][1]].max())
        gap = ints[1][0] - ints[0][1]
        if (mv < tenth or (ints[0][1] - ints[0][0] <= gap // 2 and mv < quarter)) and gap >= SPIKE_GAP:
            ints = ints[1:]
            n_removed += 1
        else:
            break
    while len(ints) > 1:
        if ints[-1][0] == ints[-1][1]:
            ints = ints[:-1]
            n_removed += 1
            continue
        mv = np.float32(y_abs[ints[-1][0]:ints[-1][1]].max())
        gap = ints[-1][0] - ints[-2][1]
        if (mv < tenth or (ints[-1][1] - ints[-1][0] <= gap // 2 and mv < quarter)) and gap >= SPIKE_GAP:
            ints = ints[:-1]
            n_removed += 1
        else:
            break
    return ints, n_removed


def trim_audio(y, gap_threshold=12288, detail=False):
    """(status, n_removed, v95, out) of one waveform; v95 and out are None where the reference has none.  With detail, a dict of the
    intermediate results is appended."""
    y = np.asarray(y, np.float32)
    d = {}

    def done(status, n_removed, v95, out):
        return (status, n_removed, v95, out, d) if detail else (status, n_removed, v95, out)

    ints, n_removed = select_intervals(y, S.split(y, *SPLIT1))
    d["kept"] = ints
    for k in range(len(ints) - 1):
        if ints[k + 1][0] - ints[k][1] >= gap_threshold:
            return done(GAP, n_removed, None, None)
    voiced = np.sort(np.abs(np.concatenate([y[l:r] for l, r in ints])))
    ref = np.float32(np.abs(y).max())
    if voiced.size == 0 or ref == 0 or voiced[int(voiced.size * 0.95)] == 0:
        return done(SILENT, n_removed, None, None)
    d["n_voiced"], d["k"], d["sorted"] = voiced.size, int(voiced.size * 0.95), voiced
    v95 = np.float32(voiced[int(voiced.size * 0.95)])
    scale = np.float32(np.float64(0.244) / np.float64(v95))
    y2 = (y * scale).astype(np.float32)[ints[0][0]:ints[-1][1]]
    assert y2.dtype == np.float32
    l, r = (int(v) for v in S.trim_index(y2, *SPLIT2))
    d.update(y2=y2, l=l, r=r, pad_left=max(0, LEAD - l), pad_right=max(0, TAIL - (len(y2) - r)))
    out = np.zeros(r - l + LEAD + TAIL, np.float32)
    a, b = max(0, l - LEAD), min(len(y2), r + TAIL)
    out[a - (l - LEAD):b - (l - LEAD)] = y2[a:b]
    if not MIN_OUT <= len(out) <= MAX_OUT:
        return done(LENGTH, n_removed, v95, out)
    return done(OK, n_removed, v95, out)


# ---------------------------------------------------------------------------------------------------------------------- fixtures
# Gated harmonic bursts over a Gaussian floor of 3e-5, the family of silence_ref.fixture_signal, laid out by hand so that every branch of
# trim_audios is taken.  tests/test_prep_host.py asserts the coverage and that no frame lies near the threshold of either split.

def _tone(n, seed):
    t = np.arange(n) / float(S.SR)
    f0 = 110.0 + 60.0 * np.sin(2 * np.pi * 0.7 * t + seed)
    ph = 2 * np.pi * np.cumsum(f0) / S.SR
    tone = sum(np.sin(h * ph) / h for h in range(1, 8))
    return tone / max(1e-9, np.abs(tone).max())


def _compose(seed, total, bursts):
    """bursts: (start, length, amplitude) of gated harmonic tones over the floor."""
    rng = np.random.default_rng(seed)
    y = FLOOR * rng.standard_normal(total)
    tone = _tone(total, seed)
    for s, n, a in bursts:
        y[s:s + n] += a * tone[s:s + n]
    return y.astype(np.float32)


def _quiet_body_with_transient(seed):
    """No padding on either side: a 64-sample full-scale transient lifts the 256-sample frame maximum about 9 dB above the 2048-sample
    frame maximum, so a 1 kHz lead-in and tail about 35 dB under the long-frame maximum is sound for the first split (-40 dB) and
    silence for the second."""
    rng = np.random.default_rng(seed)
    total, lead0, body0, body1, tail1 = 44000, 4000, 9000, 31000, 37000
    y = FLOOR * rng.standard_normal(total)
    y[body0:body1] += 0.05 * _tone(total, seed)[body0:body1]
    mid = (body0 + body1) // 2
    y[mid:mid + 64] = np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
    quiet = 0.0045 * np.sin(2 * np.pi * 1000.0 * np.arange(total) / S.SR)
    y[lead0:body0] += quiet[lead0:body0]
    y[body1:tail1] += quiet[body1:tail1]
    return y.astype(np.float32)


def _square_body(seed):
    """|y| is exactly 0.3 over the whole burst: int(N * 0.95) lands inside a run of equal values."""
    rng = np.random.default_rng(seed)
    total, s, e = 36000, 5000, 30000
    y = FLOOR * rng.standard_normal(total)
    y[s:e] = np.where((np.arange(e - s) // 40) % 2 == 0, 0.3, -0.3)
    return y.astype(np.float32)


def _clicks():
    """One full-scale sample in every 512: every frame has the same energy, so the one interval is the whole file, and more than 95 % of
    its samples are exactly zero: v95 == 0 with ref == 1."""
    y = np.zeros(20480, np.float32)
    y[::512] = 1.0
    return y


def _zero_length_tail(seed):
    """L is a multiple of the hop, and a weak 200-sample burst 500 samples before the end is counted twice by the last frame (once
    directly, once reflected) but once by the frames before it: 38.5 dB under the maximum in the last frame, 41.5 dB in the others.
    Only the last frame is non-silent there, and its interval [F - 1, F) * hop clipped to L is the zero-length [L, L]."""
    total = 34816
    y = _compose(seed, total, [(4000, 20000, 0.6)]).astype(np.float64)
    top = S.frame_mse(y, 2048, 512).max()
    y[total - 700:total - 500] = np.sqrt(top * 10 ** -3.85 * 2048 / 400)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture_named():
    """(name, float32 signal) pairs, built once."""
    body = 24000
    spike = lambda s: (s, 1200, 0.03)                            # under ref / 10 of the 0.6 body
    fx = [
        ("plain", _compose(1, 34000, [(4000, body, 0.6)])),
        ("front1", _compose(2, 44000, [spike(3000), (12000, body, 0.6)])),
        ("front2", _compose(3, 54000, [spike(3000), spike(12000), (21000, body, 0.6)])),
        ("back1", _compose(4, 44000, [(4000, body, 0.6), spike(36000)])),
        ("back2", _compose(5, 54000, [(4000, body, 0.6), spike(36000), spike(45000)])),
        ("both", _compose(6, 54000, [spike(3000), (12000, body, 0.6), spike(44000)])),
        ("front3_back1", _compose(7, 72000, [spike(3000), spike(12000), spike(21000), (30000, body, 0.6), spike(62000)])),
        ("spike_near_kept", _compose(8, 40000, [spike(3000), (6800, body, 0.6)])),
        ("short_02_removed", _compose(9, 46000, [(3000, 1000, 0.12), (14000, body, 0.6)])),
        ("long_02_kept", _compose(10, 50000, [(3000, 6000, 0.12), (15500, body, 0.6)])),
        ("gap_12288_only", _compose(11, 56000, [(4000, 16000, 0.6), (35600, 16000, 0.5)])),
        ("gap_both", _compose(12, 64000, [(4000, 16000, 0.6), (40000, 16000, 0.5)])),
        ("two_bursts_ok", _compose(13, 50000, [(4000, 16000, 0.6), (28000, 16000, 0.5)])),
        ("too_short", _compose(14, 20000, [(5000, 9000, 0.6)])),
        ("too_long", _compose(15, 328000, [(3000, 321000, 0.6)])),
        ("zeros", np.zeros(20000, np.float32)),
        ("clicks", _clicks()),
        ("no_padding", _quiet_body_with_transient(16)),
        ("tie_run", _square_body(17)),
        ("zero_length_tail", _zero_length_tail(18)),
    ]
    for _, w in fx:
        w.flags.writeable = False
    return tuple(fx)


def fixture_batch():
    return [w for _, w in fixture_named()]


@functools.lru_cache(maxsize=None)
def fixture_results(gap_threshold=12288):
    """trim_audio(..., detail=True) of every fixture signal, computed once and shared by the tests."""
    return tuple(trim_audio(w, gap_threshold, detail=True) for w in fixture_batch())


def bench_signal(n, seed):
    """The benchmark's utterance: bursts of silence_ref.fixture_signal (gaps up to 12 000 samples, so no long-gap skip at 16000)."""
    return S.fixture_signal(n, seed)
