"""fp64 NumPy restatement of librosa 0.6.0's effects.split / effects.trim and of the reference's utils.audio.trim_silence_intervals
-- the oracle of the silence tests and what `bench_trim.py --cpu-baseline` times.  Not a test module (no test_ prefix), a helper like
tests/audio_ref.py.

librosa is not available where these tests run, so no golden was generated from it: the restatement is pinned by analytic cases
(tests/test_silence_host.py), where the intervals follow by hand from the frame geometry, not by recorded librosa output.

Semantics, for a waveform y of L samples and (top_db, frame_length, hop_length):
    yp = np.pad(y, frame_length // 2, mode="reflect");  F = 1 + (len(yp) - frame_length) // hop_length
    mse[f] = mean(yp[f * hop : f * hop + frame_length] ** 2)
    db[f] = 10 log10(max(1e-10, mse[f])) - 10 log10(max(1e-10, max mse));  nonsilent[f] = db[f] > -top_db
    split: edges where nonsilent changes (frame index + 1), 0 in front if frame 0 is non-silent, F behind if the last one is;
           edges * hop clipped to L, reshaped to [n, 2]
    trim:  start = first non-silent frame * hop, end = min(L, (last non-silent frame + 1) * hop)

Also here: the fixture signals shared by the host precondition test and the GPU parity tests.
"""
import numpy as np

SR, FRAME_LENGTH_MS, FRAME_SHIFT_MS = 16000, 50, 12.5
# the reference's trim_silence_intervals, and the two parameter sets of its corpus preparation
TRIM_PARAMS = (50, int(SR / 1000 * FRAME_LENGTH_MS) * 8, int(SR / 1000 * FRAME_SHIFT_MS))
PARAM_SETS = [TRIM_PARAMS, (40, 2048, 512), (40, 256, 64)]
assert TRIM_PARAMS == (50, 6400, 200)

BAND_DB = 1e-3
FIXTURE_LENGTHS = [150, 199, 200, 1000, 3199, 3200, 6401, 39800, 123457, 199800, 219800]


def reflect_index(i, n):
    """NumPy 'reflect' padding index (no edge repeat), including the repeated reflection of a pad longer than the signal."""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def frame_mse(y, frame_length, hop_length):
    y = np.asarray(y, dtype=np.float64)
    L, pad = len(y), frame_length // 2
    yp = y[reflect_index(np.arange(-pad, L + pad), L)]
    F = 1 + (len(yp) - frame_length) // hop_length
    sq = yp * yp
    frames = np.lib.stride_tricks.sliding_window_view(sq, frame_length)[::hop_length][:F]
    assert frames.shape[0] == F
    return frames.mean(axis=1)


def frame_db(y, frame_length, hop_length):
    mse = frame_mse(y, frame_length, hop_length)
    return 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))


def nonsilent(y, top_db=60, frame_length=2048, hop_length=512):
    return frame_db(y, frame_length, hop_length) > -top_db


def frames_in_band(y, top_db, frame_length, hop_length, band=BAND_DB):
    """(number of frames whose level is within `band` dB of the threshold, distance of the nearest frame in dB)."""
    d = np.abs(frame_db(y, frame_length, hop_length) + top_db)
    return int(np.sum(d < band)), float(d.min())


def split(y, top_db=60, frame_length=2048, hop_length=512):
    ns = nonsilent(y, top_db, frame_length, hop_length)
    edges = np.flatnonzero(np.diff(ns.astype(int))) + 1
    if ns[0]:
        edges = np.concatenate([[0], edges])
    if ns[-1]:
        edges = np.concatenate([edges, [len(ns)]])
    edges = np.minimum(edges.astype(np.int64) * hop_length, len(y))
    return edges.reshape((-1, 2))


def trim_index(y, top_db=60, frame_length=2048, hop_length=512):
    nz = np.flatnonzero(nonsilent(y, top_db, frame_length, hop_length))
    if nz.size == 0:
        return np.array([0, 0], dtype=np.int64)
    return np.array([int(nz[0]) * hop_length, min(len(y), (int(nz[-1]) + 1) * hop_length)], dtype=np.int64)


def trim(y, top_db=60, frame_length=2048, hop_length=512):
    idx = trim_index(y, top_db, frame_length, hop_length)
    return np.asarray(y)[idx[0]:idx[1]], idx


def trim_silence_intervals(wav):
    wav = np.asarray(wav)
    top_db, fl, hop = TRIM_PARAMS
    return np.concatenate([wav[l:r] for l, r in split(wav, top_db, fl, hop)])


def fixture_signal(n, seed):
    """Gated gliding-harmonic bursts (amplitude 0.05 to 1.0, 1 500 to 30 000 samples long) separated by gaps of 300 to 12 000 samples,
    over a Gaussian floor of 3e-5: float32 of n samples."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(SR)
    f0 = 110.0 + 60.0 * np.sin(2 * np.pi * 0.7 * t + seed)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    tone = sum(np.sin(h * ph) / h for h in range(1, 8))
    tone /= max(1e-9, np.abs(tone).max())
    gate = np.zeros(n)
    pos = int(rng.integers(0, 4000))
    while pos < n:
        burst = int(rng.integers(1500, 30001))
        gate[pos:pos + burst] = rng.uniform(0.05, 1.0)
        pos += burst + int(rng.integers(300, 12001))
    return (gate * tone + 3e-5 * rng.standard_normal(n)).astype(np.float32)


def fixture_batch(seed=100):
    return [fixture_signal(n, seed + i) for i, n in enumerate(FIXTURE_LENGTHS)]
