"""What the side benchmarks (bench_align, bench_cer, bench_dtw, bench_dur, bench_f0, bench_mcd, bench_prep, bench_resample,
bench_trim, bench_vocoder) share: importing this module puts the repository root, the package directory and tests/ (the NumPy
restatements) on sys.path, time_calls is their device-event timer and stat the JSON shape of its answer."""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "few-shot-transformer-tts_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def time_calls(fn, runs, warmup):
    """(median, min, max) in ms of `runs` calls of fn between two device events, after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def stat(t, key="ms", digits=4):
    """time_calls' answer as the dict a benchmark prints: the median under `key`, then ms_min and ms_max."""
    med, lo, hi = t
    return {key: round(med, digits), "ms_min": round(lo, digits), "ms_max": round(hi, digits)}
